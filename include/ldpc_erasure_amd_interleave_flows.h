/* ldpc_erasure_amd_interleave_flows.h -- interleaving depth on the multi-flow wire: the multi-flow sender
 * (ldpc_erasure_amd_sender_flows.h) with every flow's blocks interleaved to depth D, and the windowed multi-flow receiver
 * (ldpc_erasure_amd_rx_window_flows.h, ldpc_erasure_amd_rx_window_flows_mixed.h) created with a depth.  The order inside a flow
 * and the receiver rule are those of ldpc_erasure_amd_interleave.h; this header composes them with the flows.  Everything here
 * is additive: every other entry point keeps its bytes.  Implemented in csrc/wire_dev.hip (layout, sender) and
 * csrc/rx_window_flows_dev.hip (receiver), same shared library.
 *
 * Why both: round-robin multiplexing spreads a burst of B packets over the A active flows, B / A rows per flow.  With many flows
 * that is already thin; with 4 or 8 flows a burst of 10 packets still lands 1 - 3 rows deep in one block of every flow, and
 * depth D thins it by another factor D.
 *
 * THE ORDER, PER FLOW.  Flow f's SUBSTREAM is exactly what ldpc_amd_fec_encode_packets_ilv_dev writes for its c_f frames from
 * block0[f] at depth D: with (first_f, stride_f) = ldpc_amd_fec_tx_ilv_layout(c_f, n, block0[f], D), row j of the flow's frame i
 * is packet first_f[i] + j stride_f[i] of the substream.  A flow's runs are the single-flow layout's, short first and last runs
 * included.
 *   LDPC_AMD_FEC_TX_SEGMENTED    the substreams back to back: for t = frame_begin[f] + i,
 *                                first[t] = n * frame_begin[f] + first_f[i], stride[t] = stride_f[i].  No further condition.  The
 *                                input of ldpc_amd_fec_rxw_flows_decode_many of a depth-D object with flow_begin = packet_begin.
 *   LDPC_AMD_FEC_TX_ROUND_ROBIN  in round q = 0, 1, ... every flow that still has a q-th packet of its substream emits it, flows
 *                                ascending.  With flow_of: the input of ldpc_amd_fec_rxw_flows_decode_mixed of a depth-D object.
 * For depth > 1 the round-robin position is affine per frame -- one first packet and one stride, the descriptor form of the
 * senders -- only when the set of active flows is constant across a run: a flow that ends inside a run of another flow changes
 * the distance between that run's rows half way.  So ROUND_ROBIN with depth > 1 needs WHOLE ALIGNED GROUPS, block0[f] % D == 0
 * and c_f % D == 0 for every flow (an empty flow is fine); otherwise LDPC_AMD_EINVAL.  Then every run is a whole group, and with
 * r = i / D, i' = i % D, A_r = the flows g with c_g > r D, rank = the flows g < f with c_g > r D and
 * base_r = n D (A_0 + ... + A_{r-1}), row j of frame i of flow f is packet base_r + rank + (j D + i') A_r:
 * first = base_r + rank + i' A_r, stride = D A_r.  depth = 1 is ldpc_amd_fec_tx_flows_layout and
 * ldpc_amd_fec_encode_packets_flows_dev byte for byte, in both orders, with any block0 and any counts.
 *
 * THE SENDER.  The contract of ldpc_amd_fec_encode_packets_flows_dev at the layout's index: every packet is byte for byte the
 * packet ldpc_amd_fec_encode_packets_dev produces for that flow alone; flow_of and packet_begin (= n * frame_begin) as there.
 * Two paths, the same bytes: FUSED exactly when ldpc_amd_fec_encode_packets_flows_dev would be fused for that code, S, knobs and
 * alignments and the largest row stride in bytes, stride * (8 + S), stays below 2^32; else COMPOSED.  The descriptors are staged
 * by the helper the other two descriptor-driven senders use: calls of all three enqueued back to back are all right.  Refusals:
 * those of ldpc_amd_fec_encode_packets_flows_dev, a depth outside {1, 2, 4, 8, 16}, and part groups in ROUND_ROBIN (the text names
 * the first offending flow); everything is checked before anything is enqueued and a refused call leaves the context usable.
 *
 * THE RECEIVER.  One depth per object.  Flow f of an object created with depth D behaves exactly like an ldpc_amd_fec_rxw host
 * object created with ldpc_amd_fec_rxw_create_depth(n, k, S, window, ahead_limit, D) and fed that flow's packets: that object is
 * the definition of the rule.  Only the plan scan looks at the depth (rxw_scan_flows_grouped in place of rxw_scan_flows, on the
 * segments or on the permutation of a mixed call); the winners' table, the move, both decode paths, the flush calls, pending,
 * state, stats, dropped and the host mirror do not depend on it -- close and flush are depth-free in the rule.  Depth 1 is
 * ldpc_amd_fec_rxw_flows_create.
 *
 * Out of scope: depth on the two-buffer ldpc_amd_fec_rx_flows (two buffers cannot hold two groups), a depth per flow,
 * ROUND_ROBIN with part groups (the position is only piecewise affine there), datagrams on the interleaved flows sender.
 */
#ifndef LDPC_ERASURE_AMD_INTERLEAVE_FLOWS_H
#define LDPC_ERASURE_AMD_INTERLEAVE_FLOWS_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_interleave.h"
#include "ldpc_erasure_amd_rx_window_flows.h"
#include "ldpc_erasure_amd_sender_flows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host arithmetic only -- no context, no device.  first[F], stride[F] (each may be NULL): row j of frame t (a position in
 * `source`) is packet first[t] + j * stride[t].  Returns F * n, or LDPC_AMD_EINVAL: the refusals of ldpc_amd_fec_tx_flows_layout,
 * block0 NULL, a depth outside the set, part groups in ROUND_ROBIN with depth > 1. */
int64_t ldpc_amd_fec_tx_flows_ilv_layout(int nflows, const int64_t *frame_begin, int n, const uint8_t *block0 /* [nflows] */, int depth,
                                         int order, int64_t *first, int32_t *stride);

/* source [F][k][S] -> packets [F*n][8+S]: ldpc_amd_fec_encode_packets_flows_dev with every flow interleaved to `depth`. */
int ldpc_amd_fec_encode_packets_flows_ilv_dev(ldpc_amd_ctx *ctx, int code, int S, int nflows, const int64_t *frame_begin /* host */,
                                              const uint8_t *source /* device */, const uint8_t *fec_class /* host [nflows] */,
                                              const uint8_t *block0 /* host [nflows] */, int order, uint8_t *packets /* device */,
                                              int32_t *flow_of /* device [F*n], may be NULL */,
                                              int64_t *packet_begin /* host [nflows+1], may be NULL */, int depth);

/* info[0]: path of the last ldpc_amd_fec_encode_packets_flows_ilv_dev call of this context (0 none yet, 1 fused, 2 composed);
 * info[1]: bytes of codeword scratch the context holds for the composed paths; info[2]: bytes of descriptor memory it holds
 * (shared with the other descriptor-driven senders); info[3]: frames of that call.  ldpc_amd_fec_sender_flows_info and
 * ldpc_amd_fec_sender_ilv_info keep reporting their own last call. */
int ldpc_amd_fec_sender_flows_ilv_info(ldpc_amd_ctx *ctx, int64_t info[4]);

/* ldpc_amd_fec_rxw_flows_create with a depth.  Refused (LDPC_AMD_EINVAL, before anything is allocated) beyond the refusals of
 * that call: a depth outside the set, depth > 1 with 2 * depth > window. */
int ldpc_amd_fec_rxw_flows_create_depth(ldpc_amd_ctx *ctx, int nflows, int n, int k, int S, int window, int ahead_limit, int depth,
                                        ldpc_amd_fec_rxw_flows **rx);
/* the depth the object was created with, -1 for a null object */
int ldpc_amd_fec_rxw_flows_depth(const ldpc_amd_fec_rxw_flows *rx);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_INTERLEAVE_FLOWS_H */
