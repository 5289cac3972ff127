// rx_window.cpp -- the windowed FEC receiver on the host: the DEFINITION of the rule (include/ldpc_erasure_amd_rx_window.h),
// of its depth-D form for a block-interleaved wire (include/ldpc_erasure_amd_interleave.h; D = 1 is the plain rule) and of the
// close rule as a value (include/ldpc_erasure_amd_rx_rule.h; no rule given = the default rule).
// Plain C++, no GPU involved; csrc/wire.cpp's two-buffer receiver is the pattern, and the W = 2, A = 0 case of this one.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "../../include/ldpc_erasure_amd_interleave.h"
#include "../../include/ldpc_erasure_amd_rx_rule.h"
#include "../../include/ldpc_erasure_amd_rx_window.h"
#include "../../include/ldpc_erasure_amd_wire.h"

struct ldpc_amd_fec_rxw {
    int n, k, S, W, A;
    int D;                                       // interleaving depth (ldpc_erasure_amd_interleave.h); 1 = the plain rule
    ldpc_amd_fec_rx_rule rule;                   // the close rule of step 3 (include/ldpc_erasure_amd_rx_rule.h)
    int base;                                    // wire block number of slot 0, -1 before the first packet
    int head;                                    // slot d lives in plane (head + d) % W
    std::vector<int> cnt;                        // [W] by slot
    std::vector<std::vector<uint8_t>> sym, er;   // [W] planes
    int64_t ahead;
    int64_t totals[5];
};

extern "C" {

// ---- the rule as a value (include/ldpc_erasure_amd_rx_rule.h) --------------------------------------------------------------------
int ldpc_amd_fec_rx_rule_default(int n, int k, ldpc_amd_fec_rx_rule *rule)
{
    if (!rule || n <= 0 || n > 65536 || k <= 0 || k >= n) return -1;
    const int kd = k + (int)lround((n - k) * 0.8), km = k + (int)lround((n - k) * 0.2);
    // c > kd && later > 10 || c > km && later > 100, on integers.  n - k <= 2 gives kd = n: `c > n` never holds, and `c >= n` adds
    // nothing to the rule's own c == n, so the threshold stays within 0 .. n
    *rule = ldpc_amd_fec_rx_rule{kd + 1 < n ? kd + 1 : n, 11, km + 1, 101};
    return 0;
}

int ldpc_amd_fec_rx_rule_mds(int n, int k, int depth, int giveup, ldpc_amd_fec_rx_rule *rule)
{
    if (!rule || n <= 0 || n > 65536 || k <= 0 || k >= n || !LDPC_AMD_FEC_ILV_DEPTH_OK(depth)) return -1;
    if (giveup < 0 || giveup > LDPC_AMD_FEC_RX_RULE_MAX_LATER) return -1;
    if (giveup == 0) giveup = depth * k / 2 > 1 ? depth * k / 2 : 1;
    *rule = ldpc_amd_fec_rx_rule{k, 1, 0, giveup};
    return 0;
}

int ldpc_amd_fec_rx_rule_check(int n, const ldpc_amd_fec_rx_rule *rule)
{
    if (!rule || n <= 0) return -1;
    const int32_t c[2] = {rule->c_hi, rule->c_lo}, l[2] = {rule->later_hi, rule->later_lo};
    for (int i = 0; i < 2; i++) {
        if (c[i] < 0 || c[i] > n || l[i] < 0 || l[i] > LDPC_AMD_FEC_RX_RULE_MAX_LATER) return -1;
        if (c[i] == 0 && l[i] < 1) return -1;   // an empty window would close on every packet and never re-anchor
    }
    return 0;
}

int ldpc_amd_fec_rxw_create(int n, int k, int S, int window, int ahead_limit, ldpc_amd_fec_rxw **out)
{
    return ldpc_amd_fec_rxw_create_rule(n, k, S, window, ahead_limit, 1, nullptr, out);
}

int ldpc_amd_fec_rxw_create_depth(int n, int k, int S, int window, int ahead_limit, int depth, ldpc_amd_fec_rxw **out)
{
    return ldpc_amd_fec_rxw_create_rule(n, k, S, window, ahead_limit, depth, nullptr, out);
}

int ldpc_amd_fec_rxw_create_rule(int n, int k, int S, int window, int ahead_limit, int depth, const ldpc_amd_fec_rx_rule *rule,
                                 ldpc_amd_fec_rxw **out)
{
    if (!LDPC_AMD_FEC_ILV_DEPTH_OK(depth) || (depth > 1 && 2 * depth > window)) return -1;
    if (!out || n <= 0 || n > 65536 || k <= 0 || k >= n || S <= 0) return -1;
    if (window < LDPC_AMD_RXW_MIN_WINDOW || window > LDPC_AMD_RXW_MAX_WINDOW || ahead_limit < 0 || ahead_limit > (1 << 30)) return -1;
    ldpc_amd_fec_rx_rule r;
    if (rule) r = *rule;
    else if (ldpc_amd_fec_rx_rule_default(n, k, &r)) return -1;
    if (ldpc_amd_fec_rx_rule_check(n, &r)) return -1;
    ldpc_amd_fec_rxw *rx = new (std::nothrow) ldpc_amd_fec_rxw();
    if (!rx) return -1;
    rx->n = n; rx->k = k; rx->S = S; rx->W = window; rx->A = ahead_limit; rx->D = depth;
    rx->rule = r;
    rx->base = -1;
    rx->head = 0;
    rx->cnt.assign((size_t)window, 0);
    rx->sym.assign((size_t)window, std::vector<uint8_t>((size_t)n * S, 0));   // payload zero, every symbol erased
    rx->er.assign((size_t)window, std::vector<uint8_t>((size_t)n, 1));
    rx->ahead = 0;
    memset(rx->totals, 0, sizeof(rx->totals));
    *out = rx;
    return 0;
}

void ldpc_amd_fec_rxw_destroy(ldpc_amd_fec_rxw *rx) { delete rx; }

int ldpc_amd_fec_rxw_depth(const ldpc_amd_fec_rxw *rx) { return rx ? rx->D : -1; }

int ldpc_amd_fec_rxw_get_rule(const ldpc_amd_fec_rxw *rx, ldpc_amd_fec_rx_rule *rule)
{
    if (!rx || !rule) return -1;
    *rule = rx->rule;
    return 0;
}

int ldpc_amd_fec_rxw_stats(const ldpc_amd_fec_rxw *rx, int64_t totals[5])
{
    if (!rx || !totals) return -1;
    memcpy(totals, rx->totals, sizeof(rx->totals));
    return 0;
}

long ldpc_amd_fec_rxw_dropped(const ldpc_amd_fec_rxw *rx)
{
    return rx ? (long)(rx->totals[LDPC_AMD_RXW_BAD_SYMBOL] + rx->totals[LDPC_AMD_RXW_LATE] + rx->totals[LDPC_AMD_RXW_AHEAD]) : -1;
}

int ldpc_amd_fec_rxw_state(const ldpc_amd_fec_rxw *rx, int *base, int *cnt, int64_t *ahead)
{
    if (!rx) return -1;
    if (base) *base = rx->base;
    if (cnt) memcpy(cnt, rx->cnt.data(), sizeof(int) * (size_t)rx->W);
    if (ahead) *ahead = rx->ahead;
    return 0;
}

static void store(ldpc_amd_fec_rxw *rx, int d, unsigned sym, const uint8_t *payload)
{
    const int p = (rx->head + d) % rx->W;
    memcpy(rx->sym[p].data() + (size_t)sym * rx->S, payload, (size_t)rx->S);
    rx->er[p][sym] = 0;
}

// hand slot 0 out, shift the slots down by one
static void close_slot0(ldpc_amd_fec_rxw *rx, uint8_t *sym_out, uint8_t *erased_out, int *block_out)
{
    const int p = rx->head;
    if (sym_out) memcpy(sym_out, rx->sym[p].data(), rx->sym[p].size());
    if (erased_out) memcpy(erased_out, rx->er[p].data(), rx->er[p].size());
    if (block_out) *block_out = rx->base;
    memset(rx->sym[p].data(), 0, rx->sym[p].size());   // the plane becomes the new last slot, empty
    memset(rx->er[p].data(), 1, rx->er[p].size());
    for (int d = 0; d + 1 < rx->W; d++) rx->cnt[d] = rx->cnt[d + 1];
    rx->cnt[rx->W - 1] = 0;
    rx->head = (rx->head + 1) % rx->W;
    rx->base = (rx->base + 1) & 0xff;
    rx->ahead = 0;
    rx->totals[LDPC_AMD_RXW_CLOSED]++;
}

int ldpc_amd_fec_rxw_push(ldpc_amd_fec_rxw *rx, const uint8_t *packet, uint8_t *sym_out, uint8_t *erased_out, int *block_out)
{
    if (!rx || !packet) return -1;
    uint64_t word = 0;
    for (int i = 0; i < 8; i++) word |= (uint64_t)packet[i] << (8 * i);
    unsigned cls, blk, sym;
    ldpc_amd_fec_header_unpack(word, &cls, &blk, &sym);
    (void)cls;
    const uint8_t *payload = packet + LDPC_AMD_FEC_HEADER_BYTES;
    if (rx->base == -1) rx->base = (int)blk - (int)blk % rx->D;        // 1. (the start of the packet's group)
    if ((int)sym >= rx->n) {                                           // 2.
        rx->totals[LDPC_AMD_RXW_BAD_SYMBOL]++;
    } else {
        const int d = ((int)blk - rx->base) & 0xff;
        if (d < rx->W) {
            store(rx, d, sym, payload);
            rx->cnt[d]++;
        } else if (rx->A > 0 && d < 128) {
            rx->ahead++;
            rx->totals[LDPC_AMD_RXW_AHEAD]++;
        } else {
            rx->totals[LDPC_AMD_RXW_LATE]++;
        }
    }
    const int c = rx->cnt[0];                                          // 3.
    const int g = rx->D - rx->base % rx->D;                            // open slots of slot 0's group; 1 when D == 1
    long later = 0, all = 0;
    for (int d = 0; d < rx->W; d++) {
        all += rx->cnt[d];
        if (d >= g) later += rx->cnt[d];
    }
    const ldpc_amd_fec_rx_rule &r = rx->rule;
    if (c == rx->n || (c >= r.c_hi && later >= r.later_hi) || (c >= r.c_lo && later >= r.later_lo)) {
        close_slot0(rx, sym_out, erased_out, block_out);
        return 1;
    }
    if (rx->A > 0 && rx->ahead > rx->A) {
        if (all == 0) {   // re-anchor: nothing is open, the window jumps to the group where the stream is
            const int d = (int)blk % rx->D;
            rx->base = (int)blk - d;
            store(rx, d, sym, payload);
            rx->cnt[d] = 1;
            rx->ahead = 0;
            rx->totals[LDPC_AMD_RXW_RESYNCS]++;
            return 0;
        }
        close_slot0(rx, sym_out, erased_out, block_out);
        return 1;
    }
    return 0;
}

int ldpc_amd_fec_rxw_push_many(ldpc_amd_fec_rxw *rx, const uint8_t *packets, long npackets, uint8_t *sym_batch,
                               uint8_t *erased_batch, int *blocks, int max_blocks, long *consumed)
{
    if (!rx || (npackets > 0 && !packets) || npackets < 0 || !sym_batch || !erased_batch || max_blocks < 1) return -1;
    const size_t plen = (size_t)LDPC_AMD_FEC_HEADER_BYTES + (size_t)rx->S, fsz = (size_t)rx->n * rx->S;
    int closed = 0;
    long i = 0;
    for (; i < npackets && closed < max_blocks; i++) {
        int blk = -1;
        if (ldpc_amd_fec_rxw_push(rx, packets + (size_t)i * plen, sym_batch + (size_t)closed * fsz, erased_batch + (size_t)closed * rx->n, &blk) == 1) {
            if (blocks) blocks[closed] = blk;
            closed++;
        }
    }
    if (consumed) *consumed = i;
    return closed;
}

int ldpc_amd_fec_rxw_flush(ldpc_amd_fec_rxw *rx, uint8_t *sym_batch, uint8_t *erased_batch, int *blocks)
{
    if (!rx) return -1;
    int count = 0;
    for (int d = 0; d < rx->W; d++)
        if (rx->cnt[d] > 0) count = d + 1;
    const size_t fsz = (size_t)rx->n * rx->S;
    for (int j = 0; j < count; j++)
        close_slot0(rx, sym_batch ? sym_batch + (size_t)j * fsz : nullptr, erased_batch ? erased_batch + (size_t)j * rx->n : nullptr,
                    blocks ? blocks + j : nullptr);
    return count;
}

}  // extern "C"
