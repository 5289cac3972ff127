/* ldpc_erasure_amd_rs_wire.h -- Reed-Solomon on the FEC wire: a sender that turns source blocks of a registered RS code into wire
 * packets, straight or block-interleaved, and an RS decode tail on the windowed device receiver.  Everything here is additive: every
 * other entry point keeps its bytes.  Implemented in csrc/rs_wire_dev.hip (the packet encoder and the row decoder), csrc/wire_dev.hip (the sender's
 * entry point) and csrc/rx_window_dev.hip (the receiver's), same shared library.
 *
 * Why: the paper's comparison of a long LDPC code with a short RS code on a bursty channel turns on interleaving -- a short RS code
 * loses "unless an interleaver is used to combine symbols across multiple RS code blocks" (Latex/Milcom_2022_ErasureCodes.tex:173), and
 * the interleaver costs the latency the short code was to save.  The wire carries LDPC streams through the link emulator
 * (ldpc_erasure_amd_link.h) and the depth-D interleaver (ldpc_erasure_amd_interleave.h); with the calls below an RS stream takes the
 * same road, so (2040,1530) LDPC at depth 1 and RS(255,192) at depth 8 -- both 2040 packets deep -- meet the same loss trace.
 *
 * THE CLASS BYTE.  The wire header carries a code class (FECClassCode, "our LDPC code is type 1",
 * ldpc_erasure_encoder_VITA_in_UDP_out.cl:58).  LDPC_AMD_FEC_CLASS_RS is the value this library's tools give RS streams.  No receiver
 * reads the byte: which decoder a stream goes to is the caller's knowledge, as it is for LDPC streams.
 *
 * THE SENDER.  rs is a handle of ldpc_amd_rs_create, (n,k) its code.  The packet at index first[b] + j stride[b] -- first and stride from
 * ldpc_amd_fec_tx_ilv_layout(nblocks, n, block0, depth) -- is byte for byte packet b n + j of the composition
 *     ldpc_amd_rs_encode_batch(ctx, rs, S, nblocks, source, cw, LDPC_AMD_DEVICE_PTRS);
 *     ldpc_amd_fec_packetize_dev(ctx, cw, nblocks, n, S, fec_class, block0, packets);
 * Depth 1 is the straight order.  Two paths, the same bytes:
 *   FUSED     one kernel (rs_encode_packets_kernel): every source row is read once, stored into its packet and multiplied into the n-k
 *             parity accumulators held in registers; the parity packets and all headers are stored by the same kernel.  Taken for
 *             S >= 16 with S a multiple of 16 (a multiple of 4 under symbol unit 4, ldpc_erasure_amd_words.h), packets 8-byte aligned,
 *             source 16-byte aligned (4-byte for the lengths only unit 4 accepts), knob ENC_PKT not 0.
 *   COMPOSED  the RS encoder into the context's codeword scratch of at most 256 MiB, chunk by chunk, then the descriptor-driven
 *             packetisers of the interleaved sender.  S = 1 is always composed.
 * The descriptors are staged as the interleaved sender stages its own (pinned slots that are not reused under a copy in flight): two
 * calls enqueued back to back are both right.  Everything is checked before anything is enqueued; a refused call leaves the context
 * usable and `packets` untouched:
 *   LDPC_AMD_ENOCODE  unknown RS handle
 *   LDPC_AMD_EINVAL   nblocks < 0, S < 1, nblocks * n >= 2^31, a depth outside 1, 2, 4, 8, 16, null or host pointers, source and
 *                     packets overlapping, a source of word-sized symbols that is not 4-byte aligned
 *   LDPC_AMD_EUNSUP   S refused by the context's symbol-length rule
 * A null context is LDPC_AMD_EINVAL before any device is touched.  nblocks == 0 is LDPC_AMD_OK and touches nothing.
 *
 * THE RECEIVER.  ldpc_amd_fec_rxw_dev_rs_decode_many is ldpc_amd_fec_rxw_dev_push_many followed by ldpc_amd_rs_decode_frames on the
 * blocks that closed, without the frames leaving the library: blocks, consumed, erased_batch, the five totals and the state are what
 * push_many gives; msg, received and status are what ldpc_amd_rs_decode_frames returns for the planes push_many would have handed out
 * (first-k selection, ReedSolomonErasureCodes.m:78-81: a block with fewer than k symbols decodes to zeros, status
 * LDPC_AMD_RS_ST_SHORT).  The receiver must have been created for the RS code's (n,k) -- any window, ahead limit and depth -- else
 * LDPC_AMD_EINVAL.  Two paths, the same bytes:
 *   FUSED     no row is copied: the receiver writes one source word per (block, symbol) -- the packet that won the symbol, the row of
 *             a staging plane, or erased -- and the decoder on rows in place (below) reads the rows where they lie, the W staging
 *             planes being one `stage` base.  Taken where that decoder applies and wins: 1 <= n - k <= 64, S >= 16 accepted by the
 *             context's symbol-length rule, packets 8-byte and msg 4-byte aligned, knob RX_PKT not 0 -- less the shapes the composed
 *             decoder streams already (n - k <= 32 with S a multiple of 256, or a word length from 256 up), where it is the faster.
 *   COMPOSED  the closed blocks are gathered chunk by chunk into the context's received-symbol scratch (at most 256 MiB), each chunk
 *             followed by the RS decoder of ldpc_amd_rs_decode_frames.  S = 1 and n - k > 64 are always composed.
 * ldpc_amd_fec_rxw_dev_rs_decode_flush is never fused, as the LDPC flush of this object is not: its blocks lie complete in their
 * planes and go through the scratch.  Every workspace is reserved before anything moves, and the staging planes are rewritten behind
 * the decode: a refused call leaves the receiver where it was.  RS calls, the LDPC decode calls, push_many and the flushes mix freely
 * on one object.
 *
 * THE DECODER ON ROWS IN PLACE.  ldpc_amd_rs_decode_rows_dev (ldpc_erasure_amd_rs_rows.h, included here) is the decoder the fused
 * receiver runs, on its own: src holds one source word per (block, symbol) -- the payload of packet p, LDPC_AMD_ROW_STAGED | i for row
 * i of `stage`, or LDPC_AMD_ROW_ERASED.  msg, received and status are what ldpc_amd_rs_decode_frames returns for the frames the words
 * describe, a word that names a packet >= npackets or a staged row >= nstage_rows taken as erased (no row outside the two arrays is
 * ever fetched); erased_out, if given, receives the flags after that vetting.  Two words may name the same row.  A plan kernel
 * selects the first k usable rows of every block, inverts the r x r system of its missing source rows once, on bytes, and writes a
 * k x r coefficient table; a streaming kernel of the sender's shape then reads every selected row once, where it lies, stores the
 * source rows and multiplies into r accumulators in registers -- as many as the block misses, by buckets of 8, 16, 24, 32, 48, 64.
 * The tables live in a context scratch of at most 256 MiB, reserved before anything is enqueued; more blocks than it holds are
 * decoded in chunks.  nblocks == 0 is LDPC_AMD_OK and touches nothing.  Refusals come before anything is enqueued and leave the
 * context usable and the outputs untouched:
 *   LDPC_AMD_ENOCODE  unknown RS handle
 *   LDPC_AMD_EINVAL   a negative count, S < 1, nblocks * n >= 2^31, npackets or nstage_rows >= 2^31, null or host pointers (packets /
 *                     stage may be NULL with a count of 0), msg overlapping packets, stage or src
 *   LDPC_AMD_EUNSUP   a shape the kernel does not take -- S = 1, S refused by the context's symbol-length rule, n - k > 64, packets
 *                     not 8-byte aligned, stage, msg or src not 4-byte aligned, knob RX_PKT 0.  This call has no composed fallback.
 * A null context is LDPC_AMD_EINVAL before any device is touched.
 *
 * THE CLOSE RULE ON SHORT BLOCKS.  A receiver made without a rule follows the default rule: it closes a block early when it holds more than k + round(0.2 (n-k)) symbols and later
 * blocks have sent more than 100 packets, or more than k + round(0.8 (n-k)) and more than 10.  For RS(255,192) these are 205 and 242 of
 * 255: on the reference's bursty channel (mean bad-state run of 10 packets) one burst takes a short block under 205 where a
 * (2040,1530) block, eight times as long, stays far above its 1632.  Such a block leaves through the ahead limit or the flush -- it is still
 * decoded if it holds k symbols -- and each forced close drops the packets that were ahead of the window.  An RS receiver wants a
 * window of at least two interleaving groups and an ahead limit sized for it -- and a close rule set from k: create it with
 * ldpc_amd_fec_rxw_dev_create_rule and the rule of ldpc_amd_fec_rx_rule_mds(n, k, depth, 0) (ldpc_erasure_amd_rx_rule.h), under
 * which a block leaves at its k-th symbol once the next group has begun, or once the stream has moved on by depth * k / 2 packets,
 * and the ahead limit is not reached.  Both RS calls work on an object of any rule.
 */
#ifndef LDPC_ERASURE_AMD_RS_WIRE_H
#define LDPC_ERASURE_AMD_RS_WIRE_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_interleave.h"
#include "ldpc_erasure_amd_rs_rows.h"
#include "ldpc_erasure_amd_rx_window.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_AMD_FEC_CLASS_RS 0x02

/* source [nblocks][k][S] -> packets [nblocks * n][8 + S], depth-D order (ldpc_amd_fec_tx_ilv_layout with the RS code's n); device
 * pointers.  See THE SENDER above. */
int ldpc_amd_fec_rs_encode_packets_dev(ldpc_amd_ctx *ctx, int rs, int S, int64_t nblocks, const uint8_t *source, unsigned fec_class,
                                       unsigned block0, int depth, uint8_t *packets);

/* info[0]: path of the last ldpc_amd_fec_rs_encode_packets_dev call of this context that sent a block (0 none yet, 1 fused,
 * 2 composed); info[1]: bytes of codeword scratch the context holds for the composed paths; info[2]: bytes of descriptor memory it
 * holds (device table and pinned staging, shared with the other descriptor-driven senders); info[3]: blocks of that call. */
int ldpc_amd_fec_rs_sender_info(ldpc_amd_ctx *ctx, int64_t info[4]);

/* push_many + ldpc_amd_rs_decode_frames on the blocks that closed.  Device pointers: packets [npackets][8 + S], msg [max_blocks][k][S],
 * received and status [max_blocks] (each may be NULL), erased_batch [max_blocks][n] (may be NULL).  blocks [max_blocks] and consumed
 * are written on the host, as by ldpc_amd_fec_rxw_dev_push_many.  Returns the number of blocks closed, or an error code. */
int ldpc_amd_fec_rxw_dev_rs_decode_many(ldpc_amd_fec_rxw_dev *rx, int rs, const uint8_t *packets, int64_t npackets, uint8_t *msg,
                                        int32_t *received, int32_t *status, uint8_t *erased_batch, int *blocks, int max_blocks,
                                        int64_t *consumed);

/* ldpc_amd_fec_rxw_dev_flush + RS decode of the 0..W blocks it hands out: msg [W][k][S], received / status [W] (may be NULL),
 * erased_batch [W][n] (may be NULL) on the device, blocks [W] on the host. */
int ldpc_amd_fec_rxw_dev_rs_decode_flush(ldpc_amd_fec_rxw_dev *rx, int rs, uint8_t *msg, int32_t *received, int32_t *status,
                                         uint8_t *erased_batch, int *blocks);

/* info[0]: blocks RS-decoded by the last such call of the context; info[1]: RS decode launches of that call; info[2]: bytes of
 * scratch it used -- received symbols (composed) or source words and per-block tables (fused); info[3]: its path (0 none yet,
 * 1 fused, 2 composed). */
int ldpc_amd_fec_rs_receiver_info(ldpc_amd_ctx *ctx, int64_t info[4]);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_RS_WIRE_H */
