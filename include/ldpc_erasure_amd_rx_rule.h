/* ldpc_erasure_amd_rx_rule.h -- the close rule of the windowed FEC receivers as a value.
 *
 * Step 3 of the windowed receiver (ldpc_erasure_amd_rx_window.h, THE RULE; at depth D ldpc_erasure_amd_interleave.h) closes slot 0
 * after a packet when, with c = cnt[0] and later = the packets stored in the later slots (at depth D: of the later GROUPS only),
 *        c == n  ||  (c >= c_hi && later >= later_hi)  ||  (c >= c_lo && later >= later_lo).
 * The four numbers are the rule.  Everything else of the receiver is as it was and takes no rule: steps 1 and 2, the ahead limit
 * with its forced close and its re-anchor, flush, one close at most per packet.  csrc/rx_window.cpp stays the definition; the two
 * device objects return its bytes under every rule.
 *
 * THE DEFAULT RULE, ldpc_amd_fec_rx_rule_default: (kd + 1, 11, km + 1, 101) with kd = k + round(0.8 (n-k)), km = k + round(0.2 (n-k)):
 * the rule of the reference's draft, `c > kd && later > 10 || c > km && later > 100`, restated on integers (n - k <= 2 makes kd = n;
 * c_hi is then n, which adds nothing to c == n, so that the default rule is a valid rule for every code).  A NULL rule means this
 * one, and the create calls without a rule make objects that behave byte for byte as before.  It suits long LDPC blocks: the
 * decoder wants clearly more than k symbols, and a block of thousands of packets reaches km + 1 under any loss it can decode from.
 *
 * THE MDS RULE, ldpc_amd_fec_rx_rule_mds: (k, 1, 0, giveup), giveup == 0 meaning max(1, depth * k / 2) (integer division).
 *   first clause    slot 0 holds k symbols and a later group has sent a packet: close.  It assumes a code that decodes from ANY k
 *                   symbols (Reed-Solomon: ldpc_erasure_amd_rs_wire.h), so nothing that arrives after the k-th helps, and a wire
 *                   that is ROUGHLY IN ORDER: once a later group has begun, slot 0's group has been sent.  Packets of the block
 *                   that arrive after the close are late.  A wire reordered over more than a group wants later_hi above 1.
 *   give-up clause  c_lo = 0: whatever slot 0 holds, it leaves once the later groups have sent `giveup` packets -- half of what a
 *                   whole group of k-symbol blocks needs at the least.  A slot 0 that cannot reach its threshold (the channel took
 *                   more than n - k of its packets) otherwise waits for the ahead limit, and every close by the ahead limit has
 *                   discarded the A + 1 packets that ran ahead of the window: on short blocks those are a large part of the next
 *                   blocks (ldpc_erasure_amd_rs_wire.h, THE CLOSE RULE ON SHORT BLOCKS).  With the clause the stream does not reach
 *                   the ahead limit while packets keep landing in the window.  A block closed by it is handed out as it is, all
 *                   erased if it is empty: exactly what a forced close hands out.
 *
 * VALID RULES.  0 <= c_* <= n, 0 <= later_* <= 2^30, and a clause with c_* == 0 needs later_* >= 1: an empty window (c = later = 0)
 * would otherwise close on every packet, and the re-anchor, which step 3 takes only when the close test fails and every count is
 * zero, could never be reached.  An invalid rule is refused by every create call (-1 by the host object, LDPC_AMD_EINVAL with a
 * message by the device objects) before anything is allocated.
 *
 * The device objects launch the plan-scan kernels they always had for an object whose rule EQUALS the default rule, whether it was
 * given as NULL or spelled out, and the ruled kernels (csrc/rx_window_scan_dev.h) for every other rule.
 */
#ifndef LDPC_ERASURE_AMD_RX_RULE_H
#define LDPC_ERASURE_AMD_RX_RULE_H

#include <stdint.h>

#include "ldpc_erasure_amd.h"
#include "ldpc_erasure_amd_rx_window.h"
#include "ldpc_erasure_amd_rx_window_flows.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t c_hi, later_hi, c_lo, later_lo;
} ldpc_amd_fec_rx_rule;

#define LDPC_AMD_FEC_RX_RULE_MAX_LATER (1 << 30)

/* Host arithmetic only.  0, or -1 for a null rule or n, k, depth, giveup outside 0 < k < n <= 65536, depth in {1, 2, 4, 8, 16},
 * 0 <= giveup <= 2^30. */
int ldpc_amd_fec_rx_rule_default(int n, int k, ldpc_amd_fec_rx_rule *rule);
int ldpc_amd_fec_rx_rule_mds(int n, int k, int depth, int giveup, ldpc_amd_fec_rx_rule *rule);
/* 0 for a valid rule of blocks of n symbols (VALID RULES above), else -1. */
int ldpc_amd_fec_rx_rule_check(int n, const ldpc_amd_fec_rx_rule *rule);

/* The create calls with a rule; rule == NULL: the default rule.  Refusals as those of the _create_depth calls, and an invalid
 * rule.  Every other call of the three objects works on an object of any rule. */
int ldpc_amd_fec_rxw_create_rule(int n, int k, int S, int window, int ahead_limit, int depth, const ldpc_amd_fec_rx_rule *rule,
                                 ldpc_amd_fec_rxw **rx);
int ldpc_amd_fec_rxw_dev_create_rule(ldpc_amd_ctx *ctx, int n, int k, int S, int window, int ahead_limit, int depth,
                                     const ldpc_amd_fec_rx_rule *rule, ldpc_amd_fec_rxw_dev **rx);
/* one rule for all flows of the object, as with the depth */
int ldpc_amd_fec_rxw_flows_create_rule(ldpc_amd_ctx *ctx, int nflows, int n, int k, int S, int window, int ahead_limit, int depth,
                                       const ldpc_amd_fec_rx_rule *rule, ldpc_amd_fec_rxw_flows **rx);
/* The rule the object follows (the default rule's four numbers for an object made without one).  0 / LDPC_AMD_OK, or -1 /
 * LDPC_AMD_EINVAL for a null argument. */
int ldpc_amd_fec_rxw_get_rule(const ldpc_amd_fec_rxw *rx, ldpc_amd_fec_rx_rule *rule);
int ldpc_amd_fec_rxw_dev_get_rule(const ldpc_amd_fec_rxw_dev *rx, ldpc_amd_fec_rx_rule *rule);
int ldpc_amd_fec_rxw_flows_get_rule(const ldpc_amd_fec_rxw_flows *rx, ldpc_amd_fec_rx_rule *rule);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_ERASURE_AMD_RX_RULE_H */
