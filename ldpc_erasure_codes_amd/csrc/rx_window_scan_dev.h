// rx_window_scan_dev.h -- the plan scan of the windowed FEC receiver (include/ldpc_erasure_amd_rx_window.h), shared by the device
// units that run it: rx_window_dev.hip on the packets of one stream, rx_window_flows_dev.hip on one segment per flow and workgroup.
// Everything here has internal linkage: each unit that includes the header gets its own copy.
#ifndef LDPC_ERASURE_AMD_RX_WINDOW_SCAN_DEV_H
#define LDPC_ERASURE_AMD_RX_WINDOW_SCAN_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ldpc_erasure_amd_interleave.h"
#include "../../include/ldpc_erasure_amd_rx_rule.h"
#include "../../include/ldpc_erasure_amd_rx_window.h"

namespace {

constexpr int kMaxW = LDPC_AMD_RXW_MAX_WINDOW;
constexpr int kScanChunk = 16;   // groups of 64 dense headers per LDS chunk; the next chunk's are in flight in registers meanwhile

// Result record of one scan (32-bit words): the end state, the totals of the call, the W counts, then one wire block number per close.
enum : int {
    R_BASE, R_AHEAD, R_CLOSES, R_ERR, R_RESYNCS, R_CONSUMED_LO, R_CONSUMED_HI, R_BAD_LO, R_BAD_HI, R_LATE_LO, R_LATE_HI, R_AHEADTOT_LO,
    R_AHEADTOT_HI, R_CNT = 16, R_WORDS = R_CNT + kMaxW
};

// ---- (b) the plan scan -----------------------------------------------------------------------------------------------------------
struct RxwRule {
    int n, kd, km, W, A;
};
struct RxwState {   // the open state a scan starts from; cnt[j] = 0 for j >= W
    int base, ahead;
    int cnt[kMaxW];
};

__device__ __forceinline__ bool rxw_close_rule(int c, int later, const RxwRule &r)
{
    return c == r.n || (c > r.kd && later > 10) || (c > r.km && later > 100);
}

// The RULED form (include/ldpc_erasure_amd_rx_rule.h): all four thresholds of step 3 are runtime values.  The objects whose rule
// is not the default rule scan with this record; the default rule keeps RxwRule, its two immediates and its kernels.  Step 3 stays a
// function of (c, later, ahead) alone, which is all the exactness argument below asks of it, and two things the body relies on hold
// for every VALID rule:
//   re-anchor      the body takes the re-anchor branch when the close test fails and every count is zero.  A clause with c_* == 0
//                  has later_* >= 1, so the close test is false on an empty window (c = later = 0, n >= 1) and the branch is reached
//                  exactly when the host reaches it.
//   close cascade  after a close by the give-up clause the slots behind may hold their threshold already and close on consecutive
//                  packets, one per packet, so a group of 64 can carry up to 64 events.  Every pass of the inner loop that finds an
//                  event resumes at start = L + 1, so a group takes at most 64 such passes and the iteration cap covers them.
struct RxwRuleV {
    int n, c_hi, later_hi, c_lo, later_lo, W, A;
};

__device__ __forceinline__ bool rxw_close_rule(int c, int later, const RxwRuleV &r)
{
    return c == r.n || (c >= r.c_hi && later >= r.later_hi) || (c >= r.c_lo && later >= r.later_lo);
}

// One wavefront; every value but the lane's own packet is wave-uniform.  For a group of 64 packets from lane `start` on:
//   is0 / isL / isA   this lane's packet goes to slot 0 / to a later slot of the window / is an ahead packet;
//   c, lt, ah         cnt[0], cnt[1] + .. + cnt[W-1] (GROUPED: cnt[g] + .. + cnt[W-1], the later groups only; isL likewise) and
//                     `ahead` after this lane's packet: the values before the group + the ballots' inclusive prefix popcounts;
//   bz                the lanes where step 3 fires after their packet; the first of them is the EVENT, a close or a re-anchor.
// Exactness: the host's decision after packet l depends on the packets before it only through (base, cnt[0], the sum of the later
// counts, ahead).  Between two events base is fixed, so every lane's class (slot d, ahead, late, bad symbol) is fixed, and each of
// the three values after packet l is its value before the group plus the matching packets among start..l -- the prefix popcount.
// Step 3 is a function of those three alone, so the first lane where it holds is the first packet after which the host acts, and
// every lane up to it is assigned as the host assigns it.  Which of the two events it is follows from the three values at that
// lane.  The event changes the state exactly as the host does and the lanes after it are evaluated again with the new state.  A
// dropped packet changes no count but is still a point where step 3 is tested, as on the host.
// The per-slot counts (needed only when a close makes slot 1 the new slot 0) are W counters in LDS, a ring like the planes: every
// assigned lane adds one to its slot's counter; an event reads and resets them between two barriers of the one-wavefront workgroup.
// The loop is bounded: every iteration assigns at least one packet, performs one event, or ends its group, so a call takes at most
// 2 npackets + max_blocks + groups iterations (a re-anchor needs A + 1 >= 2 packets); a cap on that reports R_ERR instead of spinning.
// The body is one function over a state record so that a per-flow kernel can call it with a segment and a state of its own.
//
// GROUPED: the depth-D rule of include/ldpc_erasure_amd_interleave.h (D = 2, 4, 8 or 16, 2 D <= W; the plain instantiation ignores D
// and carries none of what follows).  g = D - base % D open slots belong to the group of slot 0, and the window's counts split in
// three: c0 = cnt[0], mates = cnt[1] + .. + cnt[g-1], later = cnt[g] + .. + cnt[W-1].  A fourth ballot (isM, the group-mates) joins
// the three.  Exactness carries over: the host's decision after packet l now depends on the packets before it through (base, cnt[0],
// the mates' sum, the later groups' sum, ahead) -- the close test reads cnt[0] and the later groups' sum, the choice between a
// forced close and a re-anchor reads all three sums.  Between two events base is fixed, and so are g and every lane's class (slot 0,
// mate, later group, ahead, late, bad symbol); each of the four values after packet l is its value before the group plus the
// matching packets among start..l, a prefix popcount.  Step 3 is a function of (c, later, ahead) alone, so the first lane where it
// holds is the first packet after which the host acts; the kind of event follows from the four values at that lane.  The events
// restate the host's:
//   close, g > 1    the new slot 0 is a mate: c0 = cnt[next], mates -= c0, later is unchanged, g -= 1;
//   close, g == 1   the next group becomes the current one (base + 1 is a multiple of D, also across the 8-bit wrap, D | 256): its
//                   D counts leave `later`.  c0 = cnt[next]; slots 1 .. D-1 are read from the LDS ring, one lane each, and summed
//                   over the wave into mates; later -= c0 + mates; g = D;
//   re-anchor       every count is zero; base = the group start of the tripping packet, which goes to slot blk % D:
//                   c0 = (blk % D == 0), mates = 1 - c0, later = 0, g = D.
// cnt: LDS [kMaxW]; hbuf: LDS [kScanChunk * 64].  Rule: RxwRule, or RxwRuleV for the ruled form (deduced from r).
template <bool GROUPED, class Rule>
__device__ __forceinline__ void rxw_scan_body(const uint32_t *__restrict__ dense, int64_t np, const Rule r, int D, int max_blocks,
                                              const RxwState &st, int *cnt, uint32_t *hbuf, int32_t *__restrict__ dest,
                                              int32_t *__restrict__ res)
{
    const int lane = threadIdx.x;
    const uint64_t le = (lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1);   // lanes <= this one
    int base = st.base, ahead = st.ahead, h = 0;   // slot d's counter is cnt[(h + d) % W]
    int c0 = st.cnt[0], later = 0, own = 0;
    int g = 1, mates = 0;   // GROUPED only
    if (GROUPED) g = base < 0 ? D : D - (base & (D - 1));
#pragma unroll
    for (int j = 0; j < kMaxW; j++) {
        if (GROUPED && j > 0 && j < g) mates += st.cnt[j];
        else if (j > 0) later += st.cnt[j];
        if (lane == j) own = st.cnt[j];
    }
    if (lane < kMaxW) cnt[lane] = own;
    int closes = 0, resyncs = 0, err = 0;
    int64_t bad = 0, late = 0, aheadtot = 0, consumed = np, iters = 0;
    const int64_t iter_cap = 2 * np + (int64_t)max_blocks + (np + 63) / 64 + 1;
    bool done = false;
    uint32_t nb[kScanChunk];
#pragma unroll
    for (int u = 0; u < kScanChunk; u++) {
        const int64_t p = (int64_t)u * 64 + lane;
        nb[u] = p < np ? dense[p] : 0u;
    }
    for (int64_t base0 = 0; base0 < np && !done; base0 += 64 * kScanChunk) {
        __syncthreads();   // the chunk before has been read
#pragma unroll
        for (int u = 0; u < kScanChunk; u++) hbuf[u * 64 + lane] = nb[u];
#pragma unroll
        for (int u = 0; u < kScanChunk; u++) {   // headers of the next chunk in flight while this one is scanned
            const int64_t p = base0 + (int64_t)(kScanChunk + u) * 64 + lane;
            nb[u] = p < np ? dense[p] : 0u;
        }
        __syncthreads();
        for (int u = 0; u < kScanChunk && !done; u++) {
            const int64_t g0 = base0 + (int64_t)u * 64;
            if (g0 >= np) break;
            const int64_t p = g0 + lane;
            const bool valid = p < np;
            const uint32_t hw = hbuf[u * 64 + lane];
            const int blk = (int)(hw >> 16), sym = (int)(hw & 0xffffu);
            if (base < 0) {   // step 1: the first packet of the stream, before its symbol check
                base = __shfl(blk, 0);
                if (GROUPED) base -= base & (D - 1);   // the start of its group; g = D already
            }
            int d_out = -1;
            int start = 0;
            for (;;) {
                if (++iters > iter_cap) { err = 1; done = true; consumed = g0; break; }
                const bool live = valid && lane >= start;
                const bool ok = live && sym < r.n;
                const int d = (blk - base) & 0xff;
                const bool in = ok && d < r.W;
                const bool is0 = in && d == 0, isL = in && (GROUPED ? d >= g : d != 0);
                const bool isA = ok && !in && r.A > 0 && d < 128;
                const uint64_t b0 = __ballot(is0), bL = __ballot(isL), bA = __ballot(isA);
                uint64_t bM = 0;
                if (GROUPED) bM = __ballot(in && d != 0 && d < g);
                const int c = c0 + __popcll(b0 & le), lt = later + __popcll(bL & le), ah = ahead + __popcll(bA & le);
                const uint64_t bz = __ballot(live && (rxw_close_rule(c, lt, r) || (r.A > 0 && ah > r.A)));
                const uint64_t upto = bz ? ((bz & (0ull - bz)) << 1) - 1 : ~0ull;   // lanes up to the first event (all if none)
                const bool mine = live && ((upto >> lane) & 1);
                if (mine) d_out = in ? closes + d : -1;
                if (mine && in) {
                    const int j = h + d;
                    atomicAdd(&cnt[j >= r.W ? j - r.W : j], 1);
                }
                bad += __popcll(__ballot(mine && !ok));
                late += __popcll(__ballot(mine && ok && !in && !isA));
                aheadtot += __popcll(bA & upto);
                c0 += __popcll(b0 & upto);
                later += __popcll(bL & upto);
                ahead += __popcll(bA & upto);
                if (GROUPED) mates += __popcll(bM & upto);
                if (!bz) break;
                const int L = __ffsll((long long)bz) - 1;   // c0, later, ahead are now the values after lane L's packet
                if (!rxw_close_rule(c0, later, r) && c0 + later + (GROUPED ? mates : 0) == 0) {
                    // re-anchor: every counter is zero, the tripping packet opens slot 0 at its own block number (GROUPED: slot
                    // blk % D of a window that starts at its group)
                    base = __shfl(blk, L);
                    int dd = 0;   // GROUPED: the packet's slot in its group, the window starts at the group
                    if (GROUPED) {
                        dd = base & (D - 1);
                        base -= dd;
                        g = D;
                    }
                    if (lane == L) d_out = closes + dd;
                    if (lane == 0) {
                        int j = h;
                        if (GROUPED) {
                            j += dd;
                            if (j >= r.W) j -= r.W;
                        }
                        cnt[j] = 1;
                    }
                    c0 = dd == 0 ? 1 : 0;
                    if (GROUPED) {
                        mates = 1 - c0;
                        later = 0;
                    }
                    ahead = 0;
                    resyncs++;
                } else {
                    // close: slot 0 is handed out, the slots shift down by one
                    __syncthreads();   // the counters hold every packet assigned so far
                    const int h1 = h + 1 == r.W ? 0 : h + 1;
                    const int nc0 = cnt[h1];
                    int nm = 0;   // GROUPED, g == 1: the counts of the new slots 1 .. D-1
                    if (GROUPED && g == 1) {
                        if (lane >= 1 && lane < D) {
                            const int j = h1 + lane;   // D - 1 < W: the slot exists and is not the one handed out
                            nm = cnt[j >= r.W ? j - r.W : j];
                        }
#pragma unroll
                        for (int o = 1; o < LDPC_AMD_FEC_ILV_MAX_DEPTH; o <<= 1) nm += __shfl_xor(nm, o);
                        nm = __shfl(nm, 0);   // lanes 0 .. 15 hold the sum
                    }
                    __syncthreads();
                    if (lane == 0) {
                        cnt[h] = 0;   // the new last slot
                        res[R_WORDS + closes] = base;
                    }
                    closes++;
                    h = h1;
                    if (!GROUPED) {
                        later -= nc0;
                    } else if (g > 1) {
                        mates -= nc0;
                        g--;
                    } else {
                        mates = nm;
                        later -= nc0 + nm;
                        g = D;
                    }
                    c0 = nc0;
                    base = (base + 1) & 0xff;
                    ahead = 0;
                    if (closes == max_blocks) { consumed = g0 + L + 1; done = true; break; }
                }
                start = L + 1;
                if (start >= 64) break;
            }
            if (valid) dest[p] = d_out;
        }
    }
    __syncthreads();
    if (lane < kMaxW) {
        const int j = h + lane;
        res[R_CNT + lane] = lane < r.W ? cnt[j >= r.W ? j - r.W : j] : 0;
    }
    if (lane == 0) {
        res[R_BASE] = base; res[R_AHEAD] = ahead; res[R_CLOSES] = closes; res[R_ERR] = err; res[R_RESYNCS] = resyncs;
        res[R_CONSUMED_LO] = (int32_t)(uint32_t)consumed; res[R_CONSUMED_HI] = (int32_t)(consumed >> 32);
        res[R_BAD_LO] = (int32_t)(uint32_t)bad; res[R_BAD_HI] = (int32_t)(bad >> 32);
        res[R_LATE_LO] = (int32_t)(uint32_t)late; res[R_LATE_HI] = (int32_t)(late >> 32);
        res[R_AHEADTOT_LO] = (int32_t)(uint32_t)aheadtot; res[R_AHEADTOT_HI] = (int32_t)(aheadtot >> 32);
    }
}

// What a create call makes of its rule argument (null: the default rule): the rule the object follows, and whether it scans with
// the ruled kernels -- for every rule but the default one, spelled out or not.  -1 for an invalid rule.
inline int rxw_rule_resolve(int n, int k, const ldpc_amd_fec_rx_rule *given, ldpc_amd_fec_rx_rule *rule, bool *ruled)
{
    ldpc_amd_fec_rx_rule def;
    if (ldpc_amd_fec_rx_rule_default(n, k, &def)) return -1;
    *rule = given ? *given : def;
    if (ldpc_amd_fec_rx_rule_check(n, rule)) return -1;
    *ruled = rule->c_hi != def.c_hi || rule->later_hi != def.later_hi || rule->c_lo != def.c_lo || rule->later_lo != def.later_lo;
    return 0;
}

}  // namespace

#endif  // LDPC_ERASURE_AMD_RX_WINDOW_SCAN_DEV_H
