/* ldpc_erasure_amd_sender_flows.h -- the multi-flow sender: the source frames of many independent FEC streams encoded by one call
 * into ONE packet array, flow after flow or multiplexed round-robin, the input of the multi-flow receiver
 * (ldpc_erasure_amd_flows.h, ldpc_erasure_amd_flows_mixed.h).  Implemented in csrc/wire_dev.hip (the calls, the descriptor-driven
 * packetisers) and csrc/kernels.hip (the descriptor form of the persistent packet encoder), same shared library.
 *
 * Reference: the sender is one kernel per stream, OpenCL/device/ldpc_erasure_encoder_VITA_in_UDP_out.cl:84-129,168-211 -- it
 * computes a parity symbol, writes the FEC header and emits the packet; the block number advances once per frame (:134).  The
 * packet layout and the header are those of ldpc_erasure_amd_wire.h; VITA-49 framing and UDP headers are not produced.  The
 * reference's channel model is Gilbert-Elliott with a mean bad-state run of 10 (Matlab/Bursty_Error_Channel_Model_Generator.m:
 * 16-20): multiplexed over A active flows a burst of B lost packets costs every flow B / A symbols instead of one block B.
 *
 * THE ORDER.  The frames of all flows lie side by side in source [F][k][S]; flow f owns the frames frame_begin[f] ..
 * frame_begin[f+1]-1 (host array of nflows+1, non-decreasing, frame_begin[0] == 0, F = frame_begin[nflows]; c_f = its count).
 *   LDPC_AMD_FEC_TX_SEGMENTED    flow 0's packets as ldpc_amd_fec_encode_packets_dev writes them, then flow 1's, and so on: the
 *                                input of ldpc_amd_fec_rx_flows_decode_many with flow_begin[f] = n * frame_begin[f].
 *   LDPC_AMD_FEC_TX_ROUND_ROBIN  what a multiplexer emits that takes one packet from every flow in turn: in round q = 0, 1, ...
 *                                every flow that still has a q-th packet emits it, flows in ascending order; the q-th packet of a
 *                                flow is row q % n of its frame q / n.  With flow_of: the input of ..._decode_mixed.
 * Every stream is a whole number of frames long, so the set of active flows is constant while frame i of every flow is on the
 * wire, and the position is affine per frame: with A_i = the flows g with c_g > i, rank = the flows g < f with c_g > i and
 * base_i = n (A_0 + ... + A_{i-1}), row j of frame i of flow f is packet base_i + rank + j A_i.  Both orders are therefore one
 * form, a first packet index and a stride in packets per frame (SEGMENTED: first = frame * n, stride = 1).
 *
 * CONTRACT of ldpc_amd_fec_encode_packets_flows_dev.  Frame i of flow f carries block (block0[f] + i) & 0xff, class
 * fec_class[f], symbol number = row.  Every packet is byte for byte the packet ldpc_amd_fec_encode_packets_dev produces for that
 * flow alone with that flow's block0 and fec_class, at the index defined above.  flow_of[p] (when given) is the flow of packet p
 * in either order; packet_begin[f] (when given) = n * frame_begin[f], the packets of the flows before f.
 *   The call is asynchronous on the context's stream; two calls enqueued back to back are both right (the descriptors of a call
 * are staged in pinned memory that is not reused while its copy is in flight).  F == 0 returns OK and touches nothing; an
 * empty flow is legal.
 *   Two paths, the same bytes.  FUSED: one launch of the persistent packet encoder whose output address and header come from a
 * per-frame descriptor (16 bytes: first packet, stride, class << 8 | block).  It is taken exactly when
 * ldpc_amd_fec_encode_packets_dev would be fused for the same code, S, knobs and alignments and the stride of a frame's rows,
 * nflows * (8 + S) bytes at most, stays below 2^32.  COMPOSED: the encoder into the context's codeword scratch of at most
 * 256 MiB, in chunks of frames, then a descriptor-driven packetiser.  ldpc_amd_fec_sender_flows_info says which one ran;
 * ldpc_amd_fec_sender_info keeps reporting the last single-flow call.
 *
 * source, packets and flow_of are device pointers of the context's device; frame_begin, fec_class, block0 and packet_begin are
 * host arrays.  Errors: negative LDPC_AMD_E* codes, text in ldpc_amd_last_error(ctx); everything is checked before anything is
 * enqueued and a refused call leaves the context usable.  LDPC_AMD_EINVAL: a NULL context (before any device is touched);
 * nflows outside 1..4096; frame_begin, fec_class or block0 NULL; frame_begin not starting at 0 or decreasing; F * n >= 2^31 (the
 * receiver's bound on its packet count); an unknown order; a host pointer where a device pointer is due; flow_of not 4-byte
 * aligned; source overlapping packets, or flow_of overlapping either.  The encoder's own refusals pass through unchanged:
 * LDPC_AMD_EUNSUP for S and for a code not in triangle form, LDPC_AMD_ENOCODE, the word-symbol rules of ldpc_erasure_amd_words.h.
 */
#ifndef LDPC_ERASURE_AMD_SENDER_FLOWS_H
#define LDPC_ERASURE_AMD_SENDER_FLOWS_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_sender.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_AMD_FEC_TX_SEGMENTED 0
#define LDPC_AMD_FEC_TX_ROUND_ROBIN 1
#define LDPC_AMD_FEC_TX_MAX_FLOWS 4096

/* Host arithmetic only -- no context, no device.  first[F], stride[F]: row j of frame t (a position in `source`) is packet
 * first[t] + j * stride[t].  first and stride may each be NULL.  Returns F * n, or LDPC_AMD_EINVAL (nflows outside 1..4096,
 * n < 1, frame_begin NULL / not starting at 0 / decreasing, F * n >= 2^31, unknown order). */
int64_t ldpc_amd_fec_tx_flows_layout(int nflows, const int64_t *frame_begin, int n, int order, int64_t *first, int32_t *stride);

/* source [F][k][S] -> packets [F*n][8+S] in `order`; see the contract above. */
int ldpc_amd_fec_encode_packets_flows_dev(ldpc_amd_ctx *ctx, int code, int S, int nflows, const int64_t *frame_begin /* host */,
                                          const uint8_t *source /* device */, const uint8_t *fec_class /* host [nflows] */,
                                          const uint8_t *block0 /* host [nflows] */, int order, uint8_t *packets /* device */,
                                          int32_t *flow_of /* device [F*n], may be NULL */,
                                          int64_t *packet_begin /* host [nflows+1], may be NULL */);

/* info[0]: path of the last ldpc_amd_fec_encode_packets_flows_dev call of this context (0 none yet, 1 fused, 2 composed);
 * info[1]: bytes of codeword scratch the context holds for the composed paths; info[2]: bytes of descriptor memory it holds
 * (device table and pinned staging); info[3]: frames of that call. */
int ldpc_amd_fec_sender_flows_info(ldpc_amd_ctx *ctx, int64_t info[4]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_SENDER_FLOWS_H */
