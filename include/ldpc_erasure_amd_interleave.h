/* ldpc_erasure_amd_interleave.h -- the block-interleaved FEC wire: a sender that emits D consecutive blocks one row of each in
 * turn, and the depth-D form of the windowed receiver (ldpc_erasure_amd_rx_window.h) that reassembles such a stream.  Everything
 * here is additive: every other entry point keeps its bytes.  Implemented in csrc/wire_dev.hip (layout, sender), csrc/rx_window.cpp
 * (the host receiver, the DEFINITION of the rule) and csrc/rx_window_dev.hip (the device receiver), same shared library.
 *
 * Why: the channel the project is built around is Gilbert-Elliott with a mean bad-state run of 10 packets
 * (Matlab/Bursty_Error_Channel_Model_Generator.m:16-20).  A stream sent block after block takes a burst whole in one block.
 * ldpc_erasure_amd_sender_flows.h spreads a burst over the active flows; a single stream has no other flows, and interleaving
 * its own blocks is the standard answer: a burst of B packets costs each of the D blocks of a group about B / D rows.
 *
 * THE ORDER.  depth D is one of 1, 2, 4, 8, 16 (D divides 256, so groups survive the 8-bit wrap of the block number).  Frame f of
 * a call carries block b_f = (block0 + f) & 0xff and belongs to group b_f / D.  A RUN is a maximal set of consecutive frames of
 * one group: frames s .. s+m-1, m <= D (the first run of a call is shorter when block0 % D != 0, the last when the frames run
 * out).  A run owns the packets n s .. n (s+m) - 1, and row j of its member i is packet n s + j m + i: affine per frame,
 * first = n s + i, stride = m -- the descriptor form of the multi-flow sender.  D = 1 is the straight sender's order.
 *
 * THE SENDER.  The packet at index first[f] + j stride[f] is byte for byte packet f n + j of ldpc_amd_fec_encode_packets_dev for
 * the same code, S, source, fec_class and block0.  Two paths, the same bytes: FUSED, the persistent packet encoder on a
 * descriptor table built from the layout, taken exactly when ldpc_amd_fec_encode_packets_flows_dev would be fused for that code,
 * S, knobs and alignments; COMPOSED, the encoder into the context's codeword scratch of at most 256 MiB, chunk by chunk, then the
 * descriptor-driven packetisers.  The descriptors are staged as the multi-flow sender stages its own (pinned slots that are not
 * reused under a copy in flight): two calls enqueued back to back are both right.  Refusals and their atomicity are those of the
 * single-flow sender (everything is checked before anything is enqueued; a refused call leaves the context usable); a depth
 * outside the set and nframes * n >= 2^31 are LDPC_AMD_EINVAL; the word-symbol rules of ldpc_erasure_amd_words.h pass through.
 *
 * THE RECEIVER RULE, DEPTH D.  ldpc_erasure_amd_rx_window.h with three changes; g = D - (base mod D) is the number of open slots
 * that belong to the group of slot 0.
 *   1. base == -1: base = blk - (blk mod D), the START OF THE GROUP of the first packet.  (Anchoring on the packet's own block
 *      loses one whole block for every leading packet the link drops: its group-mates with smaller numbers are then late.)
 *   2. unchanged.
 *   3. c = cnt[0]; later = cnt[g] + ... + cnt[W-1], the packets of LATER GROUPS; all = cnt[0] + ... + cnt[W-1].
 *      The close test c == n || (c > kd && later > 10) || (c > km && later > 100) is unchanged: only `later` differs -- in an
 *      interleaved group the mates of slot 0 fill together with it and say nothing about whether slot 0 is done.
 *      A > 0 && ahead > A:  all == 0   RE-ANCHOR: base = blk - (blk mod D), the packet goes to slot blk mod D, whose count
 *                                      becomes 1; ahead = 0, resyncs++
 *                           else       CLOSE, as before.
 *   CLOSE and flush are unchanged.  With D = 1, g is always 1 and the object is ldpc_erasure_amd_rx_window.h's, byte for byte:
 *   ldpc_amd_fec_rxw_create and ldpc_amd_fec_rxw_dev_create are the D = 1 case of the calls below.
 * The window has to hold the current and the next group: depth > 1 needs 2 * depth <= window.
 *
 * WHAT DEPTH COSTS.
 *   - Latency: a block completes only when its whole group has been sent, D blocks of packets after its first row.
 *   - A stream that starts off a multiple of D: the window anchors at the group start, so up to D - 1 leading slots never
 *     receive a packet.  They are handed out as all-erased blocks, and only by forced closes (the ahead limit, or a flush).
 *   - A thin group: a block that cannot reach its threshold closes through the ahead limit, and with it each of its thin mates in
 *     turn; each forced close drops A + 1 ahead packets, so a thin group costs up to D (A + 1) where a thin block cost A + 1.
 *
 * Depth on the multi-flow sender and on the windowed multi-flow receiver: ldpc_erasure_amd_interleave_flows.h.
 */
#ifndef LDPC_ERASURE_AMD_INTERLEAVE_H
#define LDPC_ERASURE_AMD_INTERLEAVE_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_rx_window.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_AMD_FEC_ILV_MAX_DEPTH 16
/* 1, 2, 4, 8 or 16 */
#define LDPC_AMD_FEC_ILV_DEPTH_OK(d) ((d) >= 1 && (d) <= LDPC_AMD_FEC_ILV_MAX_DEPTH && ((d) & ((d) - 1)) == 0)

/* Host arithmetic only -- no context, no device.  first [nframes], stride [nframes] (each may be NULL): row j of frame f is
 * packet first[f] + j * stride[f].  Returns nframes * n, or LDPC_AMD_EINVAL (a depth outside the set, n < 1, nframes < 0,
 * nframes * n >= 2^31). */
int64_t ldpc_amd_fec_tx_ilv_layout(int64_t nframes, int n, unsigned block0, int depth, int64_t *first, int32_t *stride);

/* source [nframes][k][S] -> packets [nframes * n][8 + S] in depth-D order (device pointers); see THE SENDER above. */
int ldpc_amd_fec_encode_packets_ilv_dev(ldpc_amd_ctx *ctx, int code, int S, int64_t nframes, const uint8_t *source, unsigned fec_class,
                                        unsigned block0, int depth, uint8_t *packets);

/* info[0]: path of the last ldpc_amd_fec_encode_packets_ilv_dev call of this context (0 none yet, 1 fused, 2 composed);
 * info[1]: bytes of codeword scratch the context holds for the composed paths; info[2]: bytes of descriptor memory it holds
 * (device table and pinned staging, shared with the multi-flow sender); info[3]: frames of that call. */
int ldpc_amd_fec_sender_ilv_info(ldpc_amd_ctx *ctx, int64_t info[4]);

/* The depth-D receivers: every other call of the two objects (ldpc_erasure_amd_rx_window.h) is unchanged.  Refused (-1 /
 * LDPC_AMD_EINVAL) beyond the refusals of the plain create calls: a depth outside the set, depth > 1 with 2 * depth > window. */
int ldpc_amd_fec_rxw_create_depth(int n, int k, int S, int window, int ahead_limit, int depth, ldpc_amd_fec_rxw **rx);
int ldpc_amd_fec_rxw_dev_create_depth(ldpc_amd_ctx *ctx, int n, int k, int S, int window, int ahead_limit, int depth,
                                      ldpc_amd_fec_rxw_dev **rx);
/* the depth the object was created with, -1 for a null object */
int ldpc_amd_fec_rxw_depth(const ldpc_amd_fec_rxw *rx);
int ldpc_amd_fec_rxw_dev_depth(const ldpc_amd_fec_rxw_dev *rx);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_INTERLEAVE_H */
