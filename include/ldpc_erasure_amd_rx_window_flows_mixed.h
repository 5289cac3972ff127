/* ldpc_erasure_amd_rx_window_flows_mixed.h -- the windowed multi-flow receiver (ldpc_erasure_amd_rx_window_flows.h) fed with
 * INTERLEAVED packets: one packet array in arrival order and one flow number per packet, instead of an array the caller has
 * segmented by flow.  Implemented in csrc/rx_window_flows_dev.hip, same shared library.
 *
 * Why: the multiplexed wire of ldpc_erasure_amd_sender_flows.h (LDPC_AMD_FEC_TX_ROUND_ROBIN) and the link emulator of
 * ldpc_erasure_amd_link.h both hand on packets in arrival order with a flow_of array.  The two-buffer receiver of
 * ldpc_erasure_amd_flows_mixed.h takes that form but does not survive a reordering link (ldpc_erasure_amd_rx_window.h has the
 * figures); the windowed one survives it but took only a segmented array, so a payload sort stood between link and receiver.
 *
 * Nothing in the receiver needs a flow's packets to lie side by side: the plan reads only the header words, and the decoder and
 * the gather address a payload by packet index.  A mixed call partitions the packet INDICES by flow on the device (the stable
 * counting sort of ldpc_erasure_amd_flows_mixed.h, 4 bytes per packet; no payload byte is copied), plans every flow on the
 * permutation, and enters the packet index -- not the position -- into the winners' table, so nothing is translated back
 * afterwards.  Still one read-back and one synchronisation per call.
 *
 * CONTRACT.  Let seg_f be the packets p with flow_of[p] == f, in index order.  A mixed call returns exactly what
 * ldpc_amd_fec_rxw_flows_push_many / _decode_many return for the array seg_0 | seg_1 | ... with its flow_begin -- hence what one
 * ldpc_amd_fec_rxw host object per flow returns: the same T, closes, blocks and consumed (packets of seg_f used), every byte and
 * flag of every output array, untouched slots at and beyond T, and the same five totals, state and mirror of every flow
 * afterwards.  Duplicates stay last-copy-wins in arrival order.  Mixed calls, segmented calls and the flush calls mix freely on
 * one object.
 *   flow_of[p] outside 0 .. nflows-1 (compared unsigned, so negative values too) marks a packet of no flow ("unrouted"): it is
 * ignored and counted (ldpc_amd_fec_rxw_flows_unrouted).  offered[f] = |seg_f|.  left[p] = 1 exactly when packet p is routed and
 * its rank in its flow is >= consumed[f] -- the flow stopped at max_blocks_per_flow, the caller submits that packet again --
 * else 0.
 *   Fused or composed is chosen exactly as ldpc_amd_fec_rxw_flows_decode_many chooses for the same code, S, knobs and alignment
 * of `packets`; ldpc_amd_fec_rxw_flows_info reports it.  flow_of is read before the call returns.  Keep `packets` alive and
 * unchanged until the context's stream has passed the call.
 *   P == 0 returns 0, zeroes closes[], consumed[] and offered[] and touches (and looks at) nothing else.
 *
 * Refusals (LDPC_AMD_EINVAL), on top of those of the segmented calls: P < 0 or P >= 2^31; for P > 0 a flow_of that is NULL, in
 * host memory, or not 4-byte aligned; a `left` in host memory.  Every check and every scratch reservation comes before any state
 * changes: a refused call leaves every flow, the object (its unrouted count too) and the context where they were.  A NULL object
 * is refused (unrouted: -1) before any device is touched.  A plan scan that hits its iteration cap in ANY flow refuses the whole
 * call with LDPC_AMD_EHIP, as in the segmented calls.
 *
 * SCRATCH.  The index array (4 bytes per packet) is held by the object; the partition's table -- a histogram of [tiles][nflows]
 * 32-bit counters, at most 1024 tiles -- is the context's, shared with ldpc_erasure_amd_flows_mixed.h: at most 16 MiB + 64 KiB
 * whatever P is.
 */
#ifndef LDPC_ERASURE_AMD_RX_WINDOW_FLOWS_MIXED_H
#define LDPC_ERASURE_AMD_RX_WINDOW_FLOWS_MIXED_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_rx_window_flows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* packets: device [P][8+S], in arrival order.  flow_of: device int32 [P], 4-byte aligned; flow_of[p] in 0..nflows-1 is the flow of
 * packet p, any other value = a packet of no flow.  All other arguments, the return value and the output layout are those of
 * ldpc_amd_fec_rxw_flows_push_many / _decode_many. */
int ldpc_amd_fec_rxw_flows_push_mixed(ldpc_amd_fec_rxw_flows *rx, const uint8_t *packets, const int32_t *flow_of, int64_t P,
                                      uint8_t *sym_batch, uint8_t *erased_batch, int *blocks, int *closes, int max_blocks_per_flow,
                                      int64_t *consumed, int64_t *offered /* host [nflows], may be NULL */,
                                      uint8_t *left /* device [P], may be NULL */);
int ldpc_amd_fec_rxw_flows_decode_mixed(ldpc_amd_fec_rxw_flows *rx, int code, const uint8_t *packets, const int32_t *flow_of, int64_t P,
                                        int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                        uint8_t *erased_out, int32_t *residual_src, int *blocks, int *closes, int max_blocks_per_flow,
                                        int64_t *consumed, int64_t *offered, uint8_t *left);

/* packets of no flow that mixed calls were given so far (cumulative; -1 for NULL) */
int64_t ldpc_amd_fec_rxw_flows_unrouted(const ldpc_amd_fec_rxw_flows *rx);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_RX_WINDOW_FLOWS_MIXED_H */
