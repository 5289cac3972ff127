/* ldpc_erasure_amd_rx_window_flows.h -- the windowed multi-flow receiver: nflows windowed receivers
 * (ldpc_erasure_amd_rx_window.h) in one object, planned together like the flows of ldpc_erasure_amd_flows.h, and their batch
 * flush.  Implemented in csrc/rx_window_flows_dev.hip, same shared library.
 *
 * Why: the multi-flow receiver of ldpc_erasure_amd_flows.h restates the two-buffer close rule per flow, so ONE block of one flow
 * that ends with at most km = k + round(0.2 (n-k)) packets never closes and every later block of that flow is dropped
 * (ldpc_erasure_amd_rx_window.h has the figures).  And the windowed receiver's plan scan is one wavefront per stream: sequential
 * within a stream, independent across streams.  An object of this header keeps W blocks open PER FLOW and plans every flow at
 * once, one wavefront each.
 *
 * CONTRACT.  Flow f behaves exactly like an ldpc_amd_fec_rxw host object (csrc/rx_window.cpp, the definition of the rule) of its
 * own that is fed its segment with max_blocks = max_blocks_per_flow: the same closed blocks in the same order, block numbers,
 * bytes and flags, the same consumed[f], the same five totals, the same state afterwards.  A flow that reaches
 * max_blocks_per_flow stops consuming (consumed[f] is below its segment's length); the other flows go on; the caller submits the
 * rest of that flow again.
 *   Slot order.  Output slots are dense in flow order: all of flow 0's closed blocks in closing order, then flow 1's, and so on;
 * flow f's slots start at closes[0] + ... + closes[f-1], and blocks[] follows the same order.  push_many / decode_many return
 * the total T; slots at or beyond T are not touched.
 *   blocks, closes and consumed are final when a call returns.  Device arrays are written asynchronously on the context's
 * stream.  Keep `packets` alive and unchanged until the context's stream has passed the call.
 *   An empty segment leaves its flow untouched.  P == 0 returns 0 (closes[] and consumed[] zero) and touches nothing else.
 * All calls mix freely on one object.
 *   Flush.  For every flow of the list (NULL: all flows), in list order, flush_many hands out what ldpc_amd_fec_rxw_flush would:
 * every open slot up to the last non-empty one, 0..W blocks, empty ones in between included, each a close.  Slots are dense in
 * list order, closes[j] belongs to list entry j, the capacity is nsel * W slots.  A flow that is not listed is not touched in any
 * byte.  The flush is planned on the host from the object's mirror of the flows' states: it neither synchronises nor reads
 * anything back.
 *   Atomic refusals.  Everything is validated and every workspace reserved before any state changes: a refused call leaves every
 * flow, the object and the context as they were.  Errors are negative LDPC_AMD_E* codes with text in ldpc_amd_last_error(ctx).
 * LDPC_AMD_EINVAL: a NULL object or context (before any device is touched; dropped: -1); nflows outside 1..4096; window outside
 * 2..32; ahead_limit outside 0..2^30; nflows * window * n not below 2^31 - 2 (a staged-row word has to name the row); flow_begin
 * null, not starting at 0, or decreasing; P >= 2^31; max_blocks_per_flow < 1; nflows * max_blocks_per_flow * n not below
 * 2^31 - 2; a host pointer where a device pointer is required; a code whose (n, k) are not the object's; a flow in the flush
 * list out of range or listed twice.  Staging planes that do not fit fail create with LDPC_AMD_ENOMEM.  The decoder's own
 * refusals pass through unchanged (the word-symbol rules of ldpc_erasure_amd_words.h included).  A plan scan that hits its
 * iteration cap in ANY flow refuses the whole call with LDPC_AMD_EHIP.
 *
 * The decode calls are FUSED -- the packets-in decoder takes every row from the packets and the staging planes through its
 * row-source words (ldpc_erasure_amd_receiver.h) -- exactly where ldpc_amd_fec_rxw_dev_decode_many would be fused for the same
 * code, S, knobs and alignment of `packets` (decode_flush_many: where S is a multiple of 16 as well); else COMPOSED through the
 * context's received-symbol scratch of at most 256 MiB, in chunks of slots, one decoder launch per chunk.
 *
 * Out of scope of this header: packets interleaved with a per-packet flow number (push_mixed / decode_mixed):
 * ldpc_erasure_amd_rx_window_flows_mixed.h.
 */
#ifndef LDPC_ERASURE_AMD_RX_WINDOW_FLOWS_H
#define LDPC_ERASURE_AMD_RX_WINDOW_FLOWS_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_rx_window.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ldpc_amd_fec_rxw_flows ldpc_amd_fec_rxw_flows;

/* nflows windowed receivers for (n, k) blocks of S-byte symbols; window and ahead_limit as for ldpc_amd_fec_rxw_dev_create.
 * The staging planes, [nflows][window][n][S] and [nflows][window][n], are allocated here.  Destroy the object before its
 * context. */
int ldpc_amd_fec_rxw_flows_create(ldpc_amd_ctx *ctx, int nflows, int n, int k, int S, int window, int ahead_limit,
                                  ldpc_amd_fec_rxw_flows **out);
void ldpc_amd_fec_rxw_flows_destroy(ldpc_amd_fec_rxw_flows *rx);

/* ldpc_amd_fec_rxw_dev_push_many for every flow.  packets: device, [P][8+S]; flow f owns packets flow_begin[f] ..
 * flow_begin[f+1]-1 (host array of nflows+1, non-decreasing, flow_begin[0] == 0, P = flow_begin[nflows] < 2^31).
 * Returns the total number of closed blocks T. */
int ldpc_amd_fec_rxw_flows_push_many(ldpc_amd_fec_rxw_flows *rx, const uint8_t *packets, const int64_t *flow_begin,
                                     uint8_t *sym_batch, uint8_t *erased_batch, /* device, [nflows*max_blocks_per_flow] slots */
                                     int *blocks /* host [nflows*max_blocks_per_flow], may be NULL */,
                                     int *closes /* host [nflows], may be NULL */, int max_blocks_per_flow,
                                     int64_t *consumed /* host [nflows], may be NULL */);

/* push_many + ldpc_amd_decode_frames over all T closed blocks.  out and the result arrays hold nflows*max_blocks_per_flow
 * slots; sweeps .. residual_src may be NULL. */
int ldpc_amd_fec_rxw_flows_decode_many(ldpc_amd_fec_rxw_flows *rx, int code, const uint8_t *packets, const int64_t *flow_begin,
                                       int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                       uint8_t *erased_out, int32_t *residual_src, int *blocks, int *closes,
                                       int max_blocks_per_flow, int64_t *consumed);

/* ldpc_amd_fec_rxw_dev_flush of every listed flow.  flows: host [nsel], NULL = all flows (nsel ignored).  sym_batch /
 * erased_batch: device, nsel * window slots; blocks: host [nsel * window], closes: host [nsel], each may be NULL.  One launch
 * gathers the blocks and resets their planes.  Returns the total T. */
int ldpc_amd_fec_rxw_flows_flush_many(ldpc_amd_fec_rxw_flows *rx, const int32_t *flows, int nsel, uint8_t *sym_batch,
                                      uint8_t *erased_batch, int *blocks, int *closes);

/* flush_many + decode of the blocks it hands out; the planes are reset behind the decode. */
int ldpc_amd_fec_rxw_flows_decode_flush_many(ldpc_amd_fec_rxw_flows *rx, int code, const int32_t *flows, int nsel, int max_sweeps,
                                             int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                             uint8_t *erased_out, int32_t *residual_src, int *blocks, int *closes);

/* The open state of every flow, from the host mirror: base host [nflows] (-1: the flow has not started), cnt host
 * [nflows][window]; each may be NULL.  Returns the blocks a flush of all flows would hand out now. */
int ldpc_amd_fec_rxw_flows_pending(const ldpc_amd_fec_rxw_flows *rx, int32_t *base, int32_t *cnt);

/* ldpc_amd_fec_rxw_dev_state / _stats / _dropped of flow `flow` (dropped: -1 for a NULL object or a flow out of range). */
int ldpc_amd_fec_rxw_flows_state(const ldpc_amd_fec_rxw_flows *rx, int flow, int *base, int *cnt, int64_t *ahead);
int ldpc_amd_fec_rxw_flows_stats(const ldpc_amd_fec_rxw_flows *rx, int flow, int64_t totals[5]);
int64_t ldpc_amd_fec_rxw_flows_dropped(const ldpc_amd_fec_rxw_flows *rx, int flow);

/* info[0] = path of the last decode_many / decode_flush_many of the context (0 none yet, 1 fused, 2 composed), [1] = blocks it
 * decoded, [2] = its decoder launches, [3] = bytes of received-symbol scratch it used. */
int ldpc_amd_fec_rxw_flows_info(ldpc_amd_ctx *ctx, int64_t info[4]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_RX_WINDOW_FLOWS_H */
