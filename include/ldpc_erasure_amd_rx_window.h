/* ldpc_erasure_amd_rx_window.h -- the windowed FEC receiver: a reassembler that keeps W blocks open instead of two, and
 * resynchronises after an outage.  A host object (plain C++, csrc/rx_window.cpp) that DEFINES the rule, and a device object
 * (csrc/rx_window_dev.hip) that returns the host object's bytes for packets already in GPU memory.
 *
 * Why: the two-buffer receiver of ldpc_erasure_amd_wire.h restates the close rule of the reference's draft
 * (OpenCL/device/ldpc_erasure_decoder_with_reordering_logic.cl:139).  A current block that ends with at most
 * km = k + round(0.2 (n-k)) packets never closes under it; the next block fills, every later block is dropped, and a flush
 * leaves two empty blocks far behind the sender.  And two open blocks cannot absorb a delay spread of several blocks.
 *
 * THE RULE.  Parameters: window W (2..32 open blocks), ahead_limit A (0 .. 2^30; 0 = never resynchronise).  State: base = the wire
 * block number of slot 0 (-1 before the first packet), cnt[W] = packets stored per slot, one plane [n][S] + n flags per slot
 * (zero / erased while empty), ahead = packets seen beyond the window since the last close.  kd = k + round(0.8 (n-k)).
 * Per packet (blk, sym, payload), in this order:
 *   1. base == -1: base = blk (before the symbol check, as in the two-buffer receiver).
 *   2. sym >= n: bad_symbol++.  Else d = (blk - base) & 0xff;
 *        d < W               store into slot d (the last copy of a symbol wins, its flag is cleared), cnt[d]++ (duplicates count);
 *        A > 0 && d < 128    dropped; ahead++, ahead_total++;
 *        else                dropped; late++.
 *   3. c = cnt[0], later = cnt[1] + ... + cnt[W-1].
 *        c == n || (c > kd && later > 10) || (c > km && later > 100)                  CLOSE
 *        else if A > 0 && ahead > A:   c + later == 0                                 RE-ANCHOR: base = blk, the packet (an ahead
 *                                                                                     packet, so sym < n) goes to slot 0, cnt[0] = 1,
 *                                                                                     ahead = 0, resyncs++; no block is handed out
 *                                      else                                           CLOSE, even when slot 0 is empty (the caller
 *                                                                                     sees the gap as an all-erased block)
 *      CLOSE: hand out slot 0 (plane, flags, block number base), shift the slots down by one, the new last slot is empty,
 *      base = (base + 1) & 0xff, ahead = 0, closed++.  A packet closes at most one block; step 3 also runs after dropped packets.
 * With W = 2 and A = 0 this is the two-buffer receiver: the same closed blocks, bytes, flags, block numbers, consumed and dropped.
 *
 * The re-anchor trusts the header of the packet that trips it: a foreign block number there mis-anchors the window until the
 * next trip (A + 1 further packets ahead of it).
 *
 * Out of scope here: many flows per object and their batch flush -- ldpc_erasure_amd_rx_window_flows.h has both; a wire whose
 * blocks are interleaved -- ldpc_erasure_amd_interleave.h has the depth-D form of both objects (the ones here are its depth 1);
 * other thresholds in step 3's close test -- ldpc_erasure_amd_rx_rule.h has the rule as a value (the objects here follow its
 * default rule, the one written out above).
 */
#ifndef LDPC_ERASURE_AMD_RX_WINDOW_H
#define LDPC_ERASURE_AMD_RX_WINDOW_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_AMD_RXW_MIN_WINDOW 2
#define LDPC_AMD_RXW_MAX_WINDOW 32
/* indices of the totals ldpc_amd_fec_rxw_stats / ldpc_amd_fec_rxw_dev_stats fill */
#define LDPC_AMD_RXW_BAD_SYMBOL 0
#define LDPC_AMD_RXW_LATE 1
#define LDPC_AMD_RXW_AHEAD 2
#define LDPC_AMD_RXW_RESYNCS 3
#define LDPC_AMD_RXW_CLOSED 4 /* blocks handed out, those of flush included */

/* ---- the host object: packets, planes and flags in host memory.  0 / -1 like ldpc_erasure_amd_wire.h. ---- */
typedef struct ldpc_amd_fec_rxw ldpc_amd_fec_rxw;
int ldpc_amd_fec_rxw_create(int n, int k, int S, int window, int ahead_limit, ldpc_amd_fec_rxw **rx);
void ldpc_amd_fec_rxw_destroy(ldpc_amd_fec_rxw *rx);
/* One packet (8 + S bytes): 1 when it closed a block (copied to sym_out [n][S] / erased_out [n] / *block_out, each may be
 * null), 0 when not, -1 on bad arguments. */
int ldpc_amd_fec_rxw_push(ldpc_amd_fec_rxw *rx, const uint8_t *packet, uint8_t *sym_out, uint8_t *erased_out, int *block_out);
/* The contract of ldpc_amd_fec_rx_push_many: stops after the packet that closed block max_blocks; returns the blocks closed. */
int ldpc_amd_fec_rxw_push_many(ldpc_amd_fec_rxw *rx, const uint8_t *packets, long npackets, uint8_t *sym_batch,
                               uint8_t *erased_batch, int *blocks, int max_blocks, long *consumed);
/* End of stream: hands out, in order, every open slot up to the last non-empty one -- 0..W blocks in ONE call, empty ones in
 * between included -- into sym_batch [W][n][S] / erased_batch [W][n] / blocks [W], each a close (base advances, ahead = 0).
 * Returns the number of blocks, 0 when the window is empty. */
int ldpc_amd_fec_rxw_flush(ldpc_amd_fec_rxw *rx, uint8_t *sym_batch, uint8_t *erased_batch, int *blocks);
int ldpc_amd_fec_rxw_stats(const ldpc_amd_fec_rxw *rx, int64_t totals[5]);
/* bad_symbol + late + ahead_total */
long ldpc_amd_fec_rxw_dropped(const ldpc_amd_fec_rxw *rx);
/* The open state: *base, cnt [W], *ahead (each may be null). */
int ldpc_amd_fec_rxw_state(const ldpc_amd_fec_rxw *rx, int *base, int *cnt, int64_t *ahead);

/* ---- the device object.  Device pointers only (packets, sym_batch, erased_batch, out, the result arrays); work is enqueued on
 * the context's stream; the host arrays `blocks` and `consumed`, the totals and the state are final when a call returns.
 * Argument lists and contracts follow ldpc_amd_fec_rx_dev_* (ldpc_erasure_amd_wire_dev.h) and ldpc_erasure_amd_receiver.h:
 * keep `packets` alive until the stream has passed the call.  After a call the state is what the host object's push_many
 * would have left, so the calls mix freely.  Refusals are atomic (the receiver is unchanged), return LDPC_AMD_E* and leave
 * text in ldpc_amd_last_error: host pointers, window outside 2..32, ahead_limit < 0, max_blocks < 1, npackets >= 2^31,
 * window * n beyond the 2^31 - 2 rows a staged-row word can name. ---- */
typedef struct ldpc_amd_fec_rxw_dev ldpc_amd_fec_rxw_dev;
int ldpc_amd_fec_rxw_dev_create(ldpc_amd_ctx *ctx, int n, int k, int S, int window, int ahead_limit, ldpc_amd_fec_rxw_dev **rx);
void ldpc_amd_fec_rxw_dev_destroy(ldpc_amd_fec_rxw_dev *rx);
int ldpc_amd_fec_rxw_dev_push_many(ldpc_amd_fec_rxw_dev *rx, const uint8_t *packets, int64_t npackets, uint8_t *sym_batch,
                                   uint8_t *erased_batch, int *blocks, int max_blocks, int64_t *consumed);
/* sym_batch [W][n][S], erased_batch [W][n] on the device, blocks [W] on the host.  Decided from the host's mirror of the
 * state, without a synchronisation: one launch gathers the blocks and resets their planes. */
int ldpc_amd_fec_rxw_dev_flush(ldpc_amd_fec_rxw_dev *rx, uint8_t *sym_batch, uint8_t *erased_batch, int *blocks);
/* push_many + ldpc_amd_decode_frames.  Fused (the decoder fetches its rows from the packets and the W staging planes) where
 * the decoder has that form for the code and S, else composed (gather into a scratch of at most 256 MiB, decode, chunk by
 * chunk).  out [max_blocks][n][S]; the result arrays as in ldpc_amd_decode_frames, each may be null. */
int ldpc_amd_fec_rxw_dev_decode_many(ldpc_amd_fec_rxw_dev *rx, int code, const uint8_t *packets, int64_t npackets, int max_sweeps,
                                     int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                     uint8_t *erased_out, int32_t *residual_src, int *blocks, int max_blocks, int64_t *consumed);
/* flush + decode of the 0..W blocks it hands out: out [W][n][S], the result arrays [W], blocks [W] on the host. */
int ldpc_amd_fec_rxw_dev_decode_flush(ldpc_amd_fec_rxw_dev *rx, int code, int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps,
                                      int32_t *residual, int32_t *status, uint8_t *erased_out, int32_t *residual_src, int *blocks);
int ldpc_amd_fec_rxw_dev_stats(const ldpc_amd_fec_rxw_dev *rx, int64_t totals[5]);
int64_t ldpc_amd_fec_rxw_dev_dropped(const ldpc_amd_fec_rxw_dev *rx);
int ldpc_amd_fec_rxw_dev_state(const ldpc_amd_fec_rxw_dev *rx, int *base, int *cnt, int64_t *ahead);
/* info[0] = path of the last decode_many / decode_flush of the context (0 none yet, 1 fused, 2 composed), [1] = blocks it
 * decoded, [2] = its decoder launches, [3] = bytes of received-symbol scratch it used. */
int ldpc_amd_fec_rxw_info(ldpc_amd_ctx *ctx, int64_t info[4]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_RX_WINDOW_H */
