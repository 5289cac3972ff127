/* ldpc_erasure_amd_flows.h -- the multi-flow device receiver: many independent FEC streams reassembled (and decoded) per call.
 * Implemented in csrc/wire_dev.hip, same shared library.
 *
 * Reference: the receiver is one kernel per stream, OpenCL/device/ldpc_erasure_decoder_with_reordering_logic.cl:44-141,214-243.
 * The packet layout, the header and the rule by which blocks open and close are those of ldpc_erasure_amd_wire.h /
 * ldpc_erasure_amd_wire_dev.h; the two decode paths (fused, composed) are those of ldpc_erasure_amd_receiver.h.
 *
 * The close rule of a stream is sequential, so a stream's plan is made by one wavefront.  It is independent across streams: an
 * object of this header holds nflows receivers, takes ONE packet array segmented by flow, plans every flow at once (one wavefront
 * per flow), reads the plans back with one copy and one synchronisation, and decodes every block that closed, of every flow, in
 * one decoder launch.
 *
 * CONTRACT.  Flow f behaves exactly like an ldpc_amd_fec_rx_dev of its own that is fed its segment with max_blocks =
 * max_blocks_per_flow: the same closed blocks in the same order, the same closes[f], consumed[f] and dropped count, every byte
 * and flag the same, the same state afterwards.  A flow that reaches max_blocks_per_flow stops consuming (consumed[f] is below
 * its segment's length); the other flows go on; the caller submits the remainder of that flow again.
 *   Output slots are dense in flow order: all of flow 0's closed blocks in closing order, then flow 1's, and so on; the slot
 * base of flow f is closes[0] + ... + closes[f-1], and blocks[] follows the same order.  The calls return the total T; slots at
 * or beyond T are not touched.
 *   blocks, closes and consumed are final when a call returns.  Device arrays are written asynchronously on the context's
 * stream.  The caller must keep `packets` alive and unchanged until the context's stream has passed the call.
 *   An empty segment leaves its flow untouched.  P == 0 returns 0 (closes[] and consumed[] zero) and touches nothing else.
 * push_many and decode_many can be mixed freely on one object, and so can the per-flow flushes, which work like the single-flow
 * flushes (decode_flush is composed and decodes one frame).
 *   Everything is validated and every workspace reserved before any state changes: a refused call leaves every flow where it
 * was, the object and the context untouched and usable.  A plan scan that hits its iteration cap in ANY flow refuses the whole
 * call (LDPC_AMD_EHIP).
 *
 * Every data pointer is a device pointer of the object's context (host pointers: LDPC_AMD_EINVAL); flow_begin, blocks, closes
 * and consumed are host arrays.  Errors: negative LDPC_AMD_E* codes, text in ldpc_amd_last_error(ctx).  LDPC_AMD_EINVAL:
 * nflows outside 1..4096; flow_begin null, not starting at 0, or decreasing; P >= 2^31; max_blocks_per_flow < 1;
 * nflows * max_blocks_per_flow * n or nflows * 2 * n not below 2^31 - 2; a flow index out of range; a code whose (n, k) are not
 * the object's.  The decoder's own refusals pass through unchanged (the word-symbol rules of ldpc_erasure_amd_words.h included).
 * Staging planes that do not fit fail create with LDPC_AMD_ENOMEM.  A NULL object is refused with LDPC_AMD_EINVAL (dropped: -1)
 * before any device is touched.
 */
#ifndef LDPC_ERASURE_AMD_FLOWS_H
#define LDPC_ERASURE_AMD_FLOWS_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_receiver.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ldpc_amd_fec_rx_flows ldpc_amd_fec_rx_flows;

/* nflows receivers for (n, k) blocks of S-byte symbols; n, k, S as for ldpc_amd_fec_rx_dev_create.  The staging planes,
 * [nflows][2][n][S] and [nflows][2][n], are allocated here.  Destroy the object before its context. */
int ldpc_amd_fec_rx_flows_create(ldpc_amd_ctx *ctx, int nflows, int n, int k, int S, ldpc_amd_fec_rx_flows **out);
void ldpc_amd_fec_rx_flows_destroy(ldpc_amd_fec_rx_flows *rx);

/* ldpc_amd_fec_rx_dev_push_many for every flow.  packets: device, [P][8+S]; flow f owns packets flow_begin[f] ..
 * flow_begin[f+1]-1 (host array of nflows+1, non-decreasing, flow_begin[0] == 0, P = flow_begin[nflows] < 2^31).
 * Returns the total number of closed blocks T. */
int ldpc_amd_fec_rx_flows_push_many(ldpc_amd_fec_rx_flows *rx, const uint8_t *packets, const int64_t *flow_begin,
                                    uint8_t *sym_batch, uint8_t *erased_batch, /* device, [nflows*max_blocks_per_flow] slots */
                                    int *blocks /* host [nflows*max_blocks_per_flow], may be NULL */,
                                    int *closes /* host [nflows], may be NULL */, int max_blocks_per_flow,
                                    int64_t *consumed /* host [nflows], may be NULL */);

/* ldpc_amd_fec_rx_dev_decode_many for every flow: one decoder launch over all T closed blocks.  Fused exactly when
 * ldpc_amd_fec_rx_dev_decode_many would be fused for the same code, S, knobs and alignment of `packets`; otherwise composed
 * through the context's received-symbol scratch of at most 256 MiB, in chunks of slots.  ldpc_amd_fec_receiver_info reports the
 * path, the scratch and the blocks (T) of the call.  out and the result arrays hold nflows*max_blocks_per_flow slots. */
int ldpc_amd_fec_rx_flows_decode_many(ldpc_amd_fec_rx_flows *rx, int code, const uint8_t *packets, const int64_t *flow_begin,
                                      int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                      uint8_t *erased_out, int32_t *residual_src, int *blocks, int *closes,
                                      int max_blocks_per_flow, int64_t *consumed);

/* end of one flow's stream: ldpc_amd_fec_rx_dev_flush / ldpc_amd_fec_rx_dev_decode_flush of flow `flow`.  Returns 1 and the
 * block's number in *block_out, or 0 when the flow has no open block. */
int ldpc_amd_fec_rx_flows_flush(ldpc_amd_fec_rx_flows *rx, int flow, uint8_t *sym_out, uint8_t *erased_out, int *block_out);
int ldpc_amd_fec_rx_flows_decode_flush(ldpc_amd_fec_rx_flows *rx, int flow, int code, int max_sweeps, int do_ml, uint8_t *out,
                                       int32_t *sweeps, int32_t *residual, int32_t *status, uint8_t *erased_out,
                                       int32_t *residual_src, int *block_out);

/* packets of flow `flow` that went to no block so far (-1: NULL object or flow out of range) */
int64_t ldpc_amd_fec_rx_flows_dropped(const ldpc_amd_fec_rx_flows *rx, int flow);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_FLOWS_H */
