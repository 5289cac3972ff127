/* ldpc_erasure_amd_flows_mixed.h -- the multi-flow device receiver fed with INTERLEAVED packets: one packet array in arrival order
 * and one flow number per packet, instead of an array the caller has segmented by flow (ldpc_erasure_amd_flows.h).
 * Implemented in csrc/wire_dev.hip, same shared library.
 *
 * Reference: the receiver is one kernel per stream, OpenCL/device/ldpc_erasure_decoder_with_reordering_logic.cl:44-141,214-243;
 * its FEC header {class:8 | block:8 | symbol:16} carries no flow, so the layer below, which knows the socket, has a flow number per
 * packet and nothing more.
 *
 * Nothing in the receiver needs a flow's packets to lie side by side: the plan reads only the header words, and the decoder and the
 * gather address a payload by packet index.  A mixed call therefore partitions the packet INDICES by flow on the device (a stable
 * counting sort, 4 bytes per packet; no payload byte is copied), plans on the permutation, and translates the planned positions
 * back to packet indices.  Still one read-back and one synchronisation per call.
 *
 * CONTRACT.  Let seg_f be the packets p with flow_of[p] == f, in index order.  A mixed call returns exactly what the segmented call
 * of ldpc_erasure_amd_flows.h returns for the array seg_0 | seg_1 | ... with its flow_begin: the same T, closes, blocks, consumed
 * (packets of seg_f used) and per-flow dropped counts, every byte and flag of every output array, untouched slots at and beyond T,
 * and the same state of every flow afterwards.  Mixed calls, segmented calls and the per-flow flushes can be used in any order on
 * one object.  Duplicates stay last-copy-wins in arrival order.
 *   flow_of[p] outside 0 .. nflows-1 marks a packet of no flow ("unrouted"): it is ignored and counted
 * (ldpc_amd_fec_rx_flows_unrouted).  offered[f] = |seg_f|.  left[p] = 1 exactly when packet p is routed and its rank in its flow is
 * >= consumed[f] -- the flow stopped at max_blocks_per_flow, the caller submits that packet again -- else 0.
 *   Fused or composed is chosen exactly as ldpc_amd_fec_rx_flows_decode_many chooses for the same code, S, knobs and alignment of
 * `packets`; ldpc_amd_fec_receiver_info reports it as before.  The caller must keep `packets` alive and unchanged until the
 * context's stream has passed the call; flow_of is read before the call returns.
 *   P == 0 returns 0, zeroes closes[], consumed[] and offered[] and touches (and looks at) nothing else.
 *
 * Refusals (LDPC_AMD_EINVAL, on top of those of the segmented calls): P < 0 or P >= 2^31; for P > 0 a flow_of that is NULL, in
 * host memory, or not 4-byte aligned.  Every check and every scratch reservation comes before any state changes: a refused call
 * leaves every flow, the object and the context where they were.  A NULL object is refused with LDPC_AMD_EINVAL (unrouted: -1)
 * before any device is touched.
 *
 * SCRATCH.  Beyond the index array (4 bytes per packet, held by the object) the partition keeps one table on the context: a
 * histogram of [tiles][nflows] 32-bit counters and nflows + 1 flow bases.  The number of tiles is capped at 1024 -- the tile grows
 * with P instead: tile length = max(1024, ceil(P / 1024) rounded up to a multiple of 64) packets -- so the table never exceeds
 * 1024 * 4096 * 4 bytes + 64 KiB = 16 MiB + 64 KiB, whatever P is.
 */
#ifndef LDPC_ERASURE_AMD_FLOWS_MIXED_H
#define LDPC_ERASURE_AMD_FLOWS_MIXED_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_flows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* packets: device [P][8+S], in arrival order.  flow_of: device int32 [P], 4-byte aligned; flow_of[p] in 0..nflows-1 is the flow of
 * packet p, any other value = a packet of no flow.  All other arguments, the return value and the output layout are those of
 * ldpc_amd_fec_rx_flows_push_many / _decode_many. */
int ldpc_amd_fec_rx_flows_push_mixed(ldpc_amd_fec_rx_flows *rx, const uint8_t *packets, const int32_t *flow_of, int64_t P,
                                     uint8_t *sym_batch, uint8_t *erased_batch, int *blocks, int *closes, int max_blocks_per_flow,
                                     int64_t *consumed, int64_t *offered /* host [nflows], may be NULL */,
                                     uint8_t *left /* device [P], may be NULL */);
int ldpc_amd_fec_rx_flows_decode_mixed(ldpc_amd_fec_rx_flows *rx, int code, const uint8_t *packets, const int32_t *flow_of, int64_t P,
                                       int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                       uint8_t *erased_out, int32_t *residual_src, int *blocks, int *closes, int max_blocks_per_flow,
                                       int64_t *consumed, int64_t *offered, uint8_t *left);

/* packets of no flow that mixed calls were given so far (cumulative; -1 for NULL) */
int64_t ldpc_amd_fec_rx_flows_unrouted(const ldpc_amd_fec_rx_flows *rx);

/* The partition on its own: order[q] (device uint32 [P]) = index of the q-th packet when the routed packets are listed flow by
 * flow, each flow in arrival order; counts (host int64 [nflows], may be NULL) = packets per flow.  Returns the number of routed
 * packets R; order[R .. P-1] is not written.  Synchronous.  Errors as above, and nflows outside 1..4096.
 * info: [0] tile length in packets of the last partition of the context, [1] its tiles, [2] scratch bytes held, [3] 0. */
int64_t ldpc_amd_fec_flows_demux_dev(ldpc_amd_ctx *ctx, const int32_t *flow_of, int64_t P, int nflows, uint32_t *order, int64_t *counts);
int ldpc_amd_fec_flows_demux_info(ldpc_amd_ctx *ctx, int64_t info[4]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_FLOWS_MIXED_H */
