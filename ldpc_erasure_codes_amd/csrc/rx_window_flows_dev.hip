// rx_window_flows_dev.hip -- the windowed multi-flow receiver (include/ldpc_erasure_amd_rx_window_flows.h): nflows receivers of
// rx_window_dev.hip in one object, planned together like the flows of wire_dev.hip.  The five steps, for nflows streams whose packets
// lie in one array, flow f's in begin[f] .. begin[f] + len[f] - 1:
//   (a) rxwf_headers        every packet's header -> one dense u32, one pass over the whole array (flow-agnostic)          (parallel)
//   (b) rxw_scan_flows      rxw_scan_body (rx_window_scan_dev.h) once per flow, one workgroup of one wavefront each, on the flow's
//                           segment and state: serials, and with them `dest`, are LOCAL to the flow.  ONE copy back, ONE synchronisation.
//                           rxw_scan_flows_grouped for an object of depth > 1 (include/ldpc_erasure_amd_interleave_flows.h): the only
//                           step that looks at the depth, in segmented and mixed calls alike.  rxw_scan_flows_ruled /
//                           rxw_scan_flows_grouped_ruled for an object whose close rule is not the default rule
//                           (include/ldpc_erasure_amd_rx_rule.h): the only step that looks at the rule.
//   (c) rxwf_winners        atomicMax of the GLOBAL packet index into the table [(T + W nflows)][n]                        (parallel)
//   (d) rxwf_move<1>        the T closed slots -> sym_batch / erased_batch; or rxwf_sources: WHERE the decoder finds each row
//   (e) rxwf_move<0>        the W open blocks of every flow -> their staging planes, in a launch behind (d) and the decode
// Tables.  The host takes the prefix sum of the closes: flow f's closed blocks are the global slots base[f] .. base[f] + closes[f] - 1,
// T in all.  The winners' table holds the T closed slots first, then the W open blocks of flow 0, of flow 1, ...: serial s of flow f is
// row base[f] + s for s < closes[f], else row T + W f + (s - closes[f]).  The staging planes are [nflows][W][n][S] / [nflows][W][n]:
// serial s of flow f lives in plane f W + (head[f] + s) % W, so its row i is staging row plane * n + i of ONE base -- all a row-source
// word of the packets-in decoder (internal.h, PacketRows) needs.  A serial below W was carried in from an earlier call.
// Order of (e).  A new serial s >= W takes over the plane of serial s - W of the same flow, a block (d) or the fused decode may still
// read: (e) stands behind both on the stream.  Inside (e) nothing is read from the planes: a work item writes its own piece of its
// own plane (W distinct planes per flow) from a packet or with zero, or leaves a carried row alone.
// Mixed calls (include/ldpc_erasure_amd_rx_window_flows_mixed.h): the packets lie in arrival order with a flow number each.  The
// plan runs on the PERMUTATION order[] that csrc/flows_demux_dev.h makes of the packet indices (flow by flow, arrival order inside a
// flow; the bases kernel writes every flow's begin / len into its WFlowIn on the device):
//   (a') rxwf_headers_idx   dense[q] = header word of packets[order[q]], q below the routed count (read from the device word)
//   (b)  rxw_scan_flows     unchanged, on the positions q; the nflows + 1 flow bases ride back behind the scan records in the ONE copy
//   (c') rxwf_winners<true> atomicMax of the packet index order[begin + q]: the table holds packet indices, as in a segmented call
//   (d), (e), the flush     unchanged;  rxwf_left marks the packets behind every flow's consumed prefix through order[]
// Flush: planned from the host mirror alone, one int32 plane number per handed-out slot (wire_dev.hip's batch flush).
// The host code every device receiver needs -- the argument check and the decode tail of the decode calls, the host mirror of a
// flow's window, the upload of the flush's plane numbers -- is csrc/rx_host.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "../../include/ldpc_erasure_amd_rx_window.h"
#include "../../include/ldpc_erasure_amd_rx_window_flows.h"
#include "../../include/ldpc_erasure_amd_rx_window_flows_mixed.h"
#include "../../include/ldpc_erasure_amd_interleave_flows.h"
#define LDPC_AMD_RX_HOST_WINDOWED
#include "rx_host.h"   // and with it rx_window_scan_dev.h
#include "flows_demux_dev.h"   // the partition of a mixed call, and kMaxFlows

using namespace ldpc_amd;

namespace {

constexpr int kHdr = 8;   // LDPC_AMD_FEC_HEADER_BYTES
constexpr int kThreads = 256;

inline unsigned grid_for(int64_t items)
{
    const int64_t b = (items + kThreads - 1) / kThreads;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(b, (int64_t)1 << 20));   // grid-stride loops cover the rest
}

// ---- (a) headers: only the first 32-bit half is read, as the host's ldpc_amd_fec_header_unpack does --------------------------------
template <bool ALIGNED4>
__global__ __launch_bounds__(kThreads) void rxwf_headers(const uint8_t *__restrict__ packets, int64_t np, int plen, uint32_t *__restrict__ dense)
{
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < np; p += (int64_t)gridDim.x * kThreads) {
        const uint8_t *h = packets + p * plen;
        uint32_t w;
        if (ALIGNED4) w = *reinterpret_cast<const uint32_t *>(h) & 0x00ffffffu;
        else w = (uint32_t)h[0] | (uint32_t)h[1] << 8 | (uint32_t)h[2] << 16;
        dense[p] = w;
    }
}

// (a) of a mixed call, on the permutation: dense[q] = the header word of packets[order[q]] for the *routed positions q -- the word the
// partition's bases kernel wrote, so no count comes back to the host in between
template <bool ALIGNED4>
__global__ __launch_bounds__(kThreads) void rxwf_headers_idx(const uint8_t *__restrict__ packets, const uint32_t *__restrict__ order,
                                                            const uint32_t *__restrict__ routed, int plen, uint32_t *__restrict__ dense)
{
    const int64_t nq = *routed;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kThreads) {
        const uint8_t *h = packets + (int64_t)order[q] * plen;
        uint32_t w;
        if (ALIGNED4) w = *reinterpret_cast<const uint32_t *>(h) & 0x00ffffffu;
        else w = (uint32_t)h[0] | (uint32_t)h[1] << 8 | (uint32_t)h[2] << 16;
        dense[q] = w;
    }
}

struct WFlowIn {    // written by the host before the plan: the flow's segment and the state its scan starts from
    int64_t begin, len;   // (a mixed call: written by the partition, fec_demux_bases, in positions of the permutation)
    int base, ahead;
    int cnt[kMaxW];
};
struct WFlowTab {   // written by the host behind the plan
    int64_t begin, used;   // the packets the flow consumed: begin .. begin + used - 1 (a mixed call: positions of the permutation)
    int base, closes, head, pad;   // base: the flow's first closed slot
};

// (b) grid: nflows workgroups of one wavefront, each with its own LDS; res: [nflows][R_WORDS + max_blocks]
__global__ __launch_bounds__(64) void rxw_scan_flows(const uint32_t *__restrict__ dense, const WFlowIn *__restrict__ in, RxwRule r, int max_blocks,
                                                    int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    __shared__ int cnt[kMaxW];
    __shared__ uint32_t hbuf[kScanChunk * 64];
    const WFlowIn *f = in + blockIdx.x;
    RxwState st;
    st.base = f->base; st.ahead = f->ahead;
#pragma unroll
    for (int j = 0; j < kMaxW; j++) st.cnt[j] = f->cnt[j];
    const int64_t begin = f->begin;
    rxw_scan_body<false>(dense + begin, f->len, r, 1, max_blocks, st, cnt, hbuf, dest + begin, res + (int64_t)blockIdx.x * (R_WORDS + max_blocks));
}

// slot -> flow, [T]: one workgroup per flow
__global__ __launch_bounds__(64) void rxwf_flow_slots(const WFlowTab *__restrict__ tab, int32_t *__restrict__ slot_flow)
{
    const WFlowTab f = tab[blockIdx.x];
    for (int s = threadIdx.x; s < f.closes; s += 64) slot_flow[f.base + s] = (int)blockIdx.x;
}

// (c) grid: (x, nflows); over each flow's consumed prefix only.  The packet index is the global one: the last copy wins, as on the host.
// MIXED: dense and dest are indexed by the POSITION p of the permutation, and the table takes the packet index order[p] -- what
// everything behind the table reads -- so no second pass over the (T + W nflows) n cells translates it afterwards.  That keeps the
// rule: a cell is only ever offered positions of ONE flow (its row belongs to the flow), the partition is stable, so order[] is
// strictly increasing inside a flow's segment, and the maximum over the packet indices is the packet at the maximum position -- the
// last copy in arrival order.
template <bool MIXED>
__global__ __launch_bounds__(kThreads) void rxwf_winners(const uint32_t *__restrict__ dense, const int32_t *__restrict__ dest,
                                                        const WFlowTab *__restrict__ tab, const uint32_t *__restrict__ order, int n, int W, int T,
                                                        int32_t *__restrict__ win)
{
    const WFlowTab f = tab[blockIdx.y];
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < f.used; q += (int64_t)gridDim.x * kThreads) {
        const int64_t p = f.begin + q;
        const int s = dest[p];
        if (s < 0) continue;   // dest >= 0 only for symbol < n, and s < closes + W
        const int64_t row = s < f.closes ? (int64_t)f.base + s : (int64_t)T + (int64_t)W * blockIdx.y + (s - f.closes);
        atomicMax(&win[row * n + (dense[p] & 0xffffu)], MIXED ? (int32_t)order[p] : (int32_t)p);   // a packet index is below 2^31
    }
}

// left[p] = 1 for the packets behind a flow's consumed prefix (the caller has zeroed left); grid: (x, nflows).  in[f].len is the
// partition's: the packets of flow f in the call.
__global__ __launch_bounds__(kThreads) void rxwf_left(const WFlowTab *__restrict__ tab, const WFlowIn *__restrict__ in,
                                                     const uint32_t *__restrict__ order, uint8_t *__restrict__ left)
{
    const WFlowTab f = tab[blockIdx.y];
    const int64_t len = in[blockIdx.y].len;
    for (int64_t q = f.used + (int64_t)blockIdx.x * kThreads + threadIdx.x; q < len; q += (int64_t)gridDim.x * kThreads)
        left[order[f.begin + q]] = 1;
}

struct WFlowMoveArgs {
    const uint8_t *packets;
    int64_t plen;
    const int32_t *win;         // [(T + W nflows)][n]
    const WFlowTab *tab;        // [nflows]
    const int32_t *slot_flow;   // [T]
    uint8_t *stage_sym;         // [nflows][W][n][S]
    uint8_t *stage_er;          // [nflows][W][n]
    uint8_t *sym_out;           // gather: [count][n][S], the closed slots first .. first + count - 1
    uint8_t *er_out;            // gather: [count][n]
    int n, S, W, T, nflows;
    int first, count;
};

// rxw_move for all flows.  Gather: row r is symbol i of global slot j = first + r / n, which is serial j - base[f] of flow f =
// slot_flow[j]: the last packet that went there, else -- a carried block -- its staging row, else zero and erased.  Staging update:
// row r is symbol i of open block o = 0 .. W-1 of flow f = r / (W n), its serial closes[f] + o: the last packet, else for a block
// opened in this call zero and erased; a carried block keeps its staging row.
template <bool GATHER, bool V16>
__global__ __launch_bounds__(kThreads) void rxwf_move(WFlowMoveArgs a)
{
    const int q = V16 ? a.S / 16 : a.S;   // 16-byte pieces or bytes of a row
    const int64_t rows = GATHER ? (int64_t)a.count * a.n : (int64_t)a.W * a.nflows * a.n;
    const int64_t total = rows * q;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int64_t r = t / q;
        const int c = (int)(t - r * q);
        const int64_t blk = r / a.n;
        const int i = (int)(r - blk * a.n);
        int f, s;
        int64_t wrow;
        if (GATHER) {
            wrow = a.first + blk;
            f = a.slot_flow[wrow];
            s = (int)wrow - a.tab[f].base;
        } else {
            f = (int)(blk / a.W);
            s = a.tab[f].closes + (int)(blk - (int64_t)f * a.W);
            wrow = (int64_t)a.T + blk;
        }
        const int w = a.win[wrow * a.n + i];
        const int b = (a.tab[f].head + s) % a.W;
        const bool carried = s < a.W;
        const int64_t erow = ((int64_t)f * a.W + b) * a.n + i;   // the block's staging row
        const int64_t srow = erow * a.S;
        uint8_t *dst = GATHER ? a.sym_out + r * a.S : a.stage_sym + srow;
        if (!GATHER && w < 0 && carried) continue;
        if (V16) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (w >= 0) {
                const uint2 *src = reinterpret_cast<const uint2 *>(a.packets + (int64_t)w * a.plen + kHdr + (int64_t)c * 16);
                const uint2 lo = src[0], hi = src[1];
                v = make_uint4(lo.x, lo.y, hi.x, hi.y);
            } else if (carried) {
                v = *reinterpret_cast<const uint4 *>(a.stage_sym + srow + (int64_t)c * 16);
            }
            *reinterpret_cast<uint4 *>(dst + (int64_t)c * 16) = v;
        } else {
            uint8_t v = 0;
            if (w >= 0) v = a.packets[(int64_t)w * a.plen + kHdr + c];
            else if (carried) v = a.stage_sym[srow + c];
            dst[c] = v;
        }
        if (c == 0) {
            const uint8_t e = w >= 0 ? 0 : (carried ? a.stage_er[erow] : 1);
            if (GATHER) a.er_out[r] = e;
            else a.stage_er[erow] = e;
        }
    }
}

// (d') the fused form: the gather's rule for the rows of the T closed slots as words the packets-in decoder follows, and the flags
__global__ __launch_bounds__(kThreads) void rxwf_sources(const int32_t *__restrict__ win, const uint8_t *__restrict__ stage_er,
                                                        const WFlowTab *__restrict__ tab, const int32_t *__restrict__ slot_flow, int n, int W,
                                                        int T, uint32_t *__restrict__ src, uint8_t *__restrict__ er)
{
    const int64_t total = (int64_t)T * n;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < total; r += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(r / n);
        const int i = (int)(r - (int64_t)j * n);
        const int f = slot_flow[j];
        const int s = j - tab[f].base;
        const int w = win[r];
        const int64_t row = ((int64_t)f * W + (tab[f].head + s) % W) * n + i;   // the block's staging row, < 2^31 - 2 (create)
        uint32_t word = kRowErased;
        if (w >= 0) word = (uint32_t)w;
        else if (s < W && stage_er[row] == 0) word = kRowStaged | (uint32_t)row;
        src[r] = word;
        er[r] = word == kRowErased ? 1 : 0;
    }
}

// ---- flush: every handed-out block lies complete in ONE plane; desc[j] = the plane f W + b of slot j, written by the host -----------
// Row-source words and flags of the T slots for the packets-in decoder: staged (row desc[j] * n + i of the planes' one base) or erased.
__global__ __launch_bounds__(kThreads) void rxwf_flush_sources(const int32_t *__restrict__ desc, const uint8_t *__restrict__ stage_er, int n, int T,
                                                              uint32_t *__restrict__ src, uint8_t *__restrict__ er)
{
    const int64_t total = (int64_t)T * n;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < total; r += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(r / n);
        const int i = (int)(r - (int64_t)j * n);
        const int64_t row = (int64_t)desc[j] * n + i;
        const uint8_t e = stage_er[row];
        src[r] = e ? kRowErased : (kRowStaged | (uint32_t)row);
        er[r] = e;
    }
}

// Slots first .. first + count - 1, grid (x, slots): COPY: plane -> dense slot; and the plane back to symbols 0 / flags 1 in the same
// work item that read it.  One work item per piece of PW bytes (16 or 1; PW divides S, so a plane has at least n pieces: piece u < n
// also moves flag u).  Each piece and flag is read and rewritten by one work item only; a plane belongs to one slot (no flow twice).
template <int PW, bool COPY>
__global__ __launch_bounds__(kThreads) void rxwf_flush_move(const int32_t *__restrict__ desc, uint8_t *__restrict__ stage_sym,
                                                           uint8_t *__restrict__ stage_er, int n, int S, int first, int count,
                                                           uint8_t *__restrict__ sym_out, uint8_t *__restrict__ er_out)
{
    const int64_t upp = (int64_t)n * S / PW;   // pieces of a plane
    for (int64_t s = blockIdx.y; s < count; s += gridDim.y) {
        const int64_t plane = desc[first + s];
        uint8_t *from = stage_sym + plane * upp * PW;
        uint8_t *to = COPY ? sym_out + s * upp * PW : nullptr;
        for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < upp; u += (int64_t)gridDim.x * kThreads) {
            if (PW == 16) {
                if (COPY) reinterpret_cast<uint4 *>(to)[u] = reinterpret_cast<const uint4 *>(from)[u];
                reinterpret_cast<uint4 *>(from)[u] = make_uint4(0, 0, 0, 0);
            } else {
                if (COPY) to[u] = from[u];
                from[u] = 0;
            }
            if (u < n) {
                if (COPY) er_out[s * n + u] = stage_er[plane * n + u];
                stage_er[plane * n + u] = 1;
            }
        }
    }
}

// (b) for an object of depth D > 1 (include/ldpc_erasure_amd_interleave_flows.h): rxw_scan_flows with the depth-D rule.  It stands
// behind the other kernels of the unit so that theirs keep their places in the code object.
__global__ __launch_bounds__(64) void rxw_scan_flows_grouped(const uint32_t *__restrict__ dense, const WFlowIn *__restrict__ in, RxwRule r, int D,
                                                            int max_blocks, int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    __shared__ int cnt[kMaxW];
    __shared__ uint32_t hbuf[kScanChunk * 64];
    const WFlowIn *f = in + blockIdx.x;
    RxwState st;
    st.base = f->base; st.ahead = f->ahead;
#pragma unroll
    for (int j = 0; j < kMaxW; j++) st.cnt[j] = f->cnt[j];
    const int64_t begin = f->begin;
    rxw_scan_body<true>(dense + begin, f->len, r, D, max_blocks, st, cnt, hbuf, dest + begin, res + (int64_t)blockIdx.x * (R_WORDS + max_blocks));
}

// (b) for an object whose close rule is not the default rule (include/ldpc_erasure_amd_rx_rule.h): the two scans above with step 3's
// four thresholds read from the argument.  Behind every other kernel of the unit, for the same reason.
__global__ __launch_bounds__(64) void rxw_scan_flows_ruled(const uint32_t *__restrict__ dense, const WFlowIn *__restrict__ in, RxwRuleV r,
                                                          int max_blocks, int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    __shared__ int cnt[kMaxW];
    __shared__ uint32_t hbuf[kScanChunk * 64];
    const WFlowIn *f = in + blockIdx.x;
    RxwState st;
    st.base = f->base; st.ahead = f->ahead;
#pragma unroll
    for (int j = 0; j < kMaxW; j++) st.cnt[j] = f->cnt[j];
    const int64_t begin = f->begin;
    rxw_scan_body<false>(dense + begin, f->len, r, 1, max_blocks, st, cnt, hbuf, dest + begin, res + (int64_t)blockIdx.x * (R_WORDS + max_blocks));
}

__global__ __launch_bounds__(64) void rxw_scan_flows_grouped_ruled(const uint32_t *__restrict__ dense, const WFlowIn *__restrict__ in, RxwRuleV r,
                                                                  int D, int max_blocks, int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    __shared__ int cnt[kMaxW];
    __shared__ uint32_t hbuf[kScanChunk * 64];
    const WFlowIn *f = in + blockIdx.x;
    RxwState st;
    st.base = f->base; st.ahead = f->ahead;
#pragma unroll
    for (int j = 0; j < kMaxW; j++) st.cnt[j] = f->cnt[j];
    const int64_t begin = f->begin;
    rxw_scan_body<true>(dense + begin, f->len, r, D, max_blocks, st, cnt, hbuf, dest + begin, res + (int64_t)blockIdx.x * (R_WORDS + max_blocks));
}

}  // namespace

struct ldpc_amd_fec_rxw_flows {
    ldpc_amd_ctx *ctx = nullptr;
    int nflows = 0, n = 0, k = 0, S = 0, W = 0, A = 0, kd = 0, km = 0;
    int D = 1;   // interleaving depth (include/ldpc_erasure_amd_interleave_flows.h); only the plan scan looks at it
    ldpc_amd_fec_rx_rule rule{};   // the close rule of every flow (include/ldpc_erasure_amd_rx_rule.h); only the plan scan looks at it
    bool ruled = false;            // the rule is not the default rule: the ruled scan kernels (else kd, km and the kernels there always were)
    // host mirror of every flow's state, as in ldpc_amd_fec_rxw_dev; head: staging plane (of the flow's W) of slot 0
    std::vector<int> base, head, ahead;
    std::vector<int> cnt;           // [nflows][W]
    std::vector<int64_t> totals;    // [nflows][5]
    int64_t unrouted = 0;           // packets of no flow the mixed calls were given
    uint8_t *stage_sym = nullptr;   // [nflows][W][n][S]
    uint8_t *stage_er = nullptr;    // [nflows][W][n]
    Scratch dense, dest, win, res, slots, order;   // per-call scratch, grown on demand (order: the mixed calls' partition, u32 [P])
    WFlowIn *in_dev = nullptr, *in_host = nullptr;      // [nflows]; the host copies are pinned
    WFlowTab *tab_dev = nullptr, *tab_host = nullptr;   // [nflows]
    int32_t *res_host = nullptr;    // pinned copy of res
    size_t res_host_cap = 0;
    RxPlaneUpload fl;   // the flush: the handed-out slots' planes on the device, [W nflows]
};

namespace {

typedef ldpc_amd_fec_rxw_flows Rx;

// One call's PLAN for all flows: (a) + (b), ONE read-back, the slot bases.  Nothing of any flow's state changes before rxwf_commit.
struct WFlowsPlan {
    int T = 0;             // closed blocks of all flows
    int64_t max_used = 0;  // the longest consumed prefix
    size_t rec = 0;        // words of one flow's result record
    // a mixed call (else null / 0): the partition, the flow bases as read back behind the scan records ([nflows + 1], the last one =
    // the routed packets), the longest remainder behind a consumed prefix
    const uint32_t *order = nullptr, *base = nullptr;
    int64_t max_left = 0;
};

inline RxwMirror rxwf_mirror(Rx *rx, int f)
{
    return RxwMirror{&rx->base[f], &rx->head[f], &rx->ahead[f], &rx->cnt[(size_t)f * rx->W], &rx->totals[(size_t)f * 5], rx->W};
}

int rxwf_check_limits(Rx *rx, const char *who, int64_t P, int max_blocks)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (P < 0 || P >= ((int64_t)1 << 31)) return set_error(ctx, LDPC_AMD_EINVAL, "%s: need fewer than 2^31 packets in all", who);
    if (max_blocks < 1) return set_error(ctx, LDPC_AMD_EINVAL, "%s: need max_blocks_per_flow >= 1", who);
    if ((int64_t)rx->nflows * max_blocks * rx->n >= ((int64_t)1 << 31) - 2)
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: nflows * max_blocks_per_flow * n must be below 2^31 - 2", who);
    return LDPC_AMD_OK;
}

int rxwf_check_call(Rx *rx, const char *who, const int64_t *flow_begin, int max_blocks, int64_t &P)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (!flow_begin || flow_begin[0] != 0) return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow_begin must not be null and must start at 0", who);
    for (int f = 0; f < rx->nflows; f++)
        if (flow_begin[f + 1] < flow_begin[f]) return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow_begin decreases at flow %d", who, f);
    P = flow_begin[rx->nflows];
    return rxwf_check_limits(rx, who, P, max_blocks);
}

// Where the packets of a call are: segmented by the caller (flow_begin, host) or interleaved with a flow number each (flow_of, device)
struct WFlowsSrc {
    bool mixed = false;
    const int64_t *flow_begin = nullptr;
    const int32_t *flow_of = nullptr;
};

// the mixed calls' own arguments, P > 0 (the device is set)
int rxwf_check_mixed(Rx *rx, const char *who, const int32_t *flow_of, const uint8_t *left)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (!flow_of || !is_device_ptr(ctx, flow_of))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow_of must be a device pointer of device %d", who, ctx->device);
    if ((uintptr_t)flow_of & 3) return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow_of must be 4-byte aligned", who);
    if (left && !is_device_ptr(ctx, left)) return set_error(ctx, LDPC_AMD_EINVAL, "%s: left must be a device pointer of device %d", who, ctx->device);
    return LDPC_AMD_OK;
}

void rxwf_nothing(const Rx *rx, int *closes, int64_t *consumed, int64_t *offered)
{
    if (closes) std::fill(closes, closes + rx->nflows, 0);
    if (consumed) std::fill(consumed, consumed + rx->nflows, (int64_t)0);
    if (offered) std::fill(offered, offered + rx->nflows, (int64_t)0);
}

int rxwf_plan(Rx *rx, const char *who, const uint8_t *packets, const WFlowsSrc &src, int64_t npackets, int max_blocks, WFlowsPlan &pl)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n, nf = rx->nflows, W = rx->W;
    const int64_t plen = (int64_t)rx->S + kHdr;
    const int64_t *flow_begin = src.flow_begin;
    const bool mixed = src.mixed;
    pl.rec = (size_t)R_WORDS + (size_t)max_blocks;
    const size_t res_bytes = sizeof(int32_t) * (pl.rec * (size_t)nf + (mixed ? (size_t)nf + 1 : 0));   // mixed: the flow bases behind the records
    int rc;
    if ((rc = scratch_reserve(ctx, rx->dense, sizeof(uint32_t) * (size_t)npackets)) ||
        (rc = scratch_reserve(ctx, rx->dest, sizeof(int32_t) * (size_t)npackets)) || (rc = scratch_reserve(ctx, rx->res, res_bytes)))
        return rc;
    if (mixed && ((rc = scratch_reserve(ctx, rx->order, sizeof(uint32_t) * (size_t)npackets)) || (rc = demux_reserve(ctx, npackets, nf)))) return rc;
    if (rx->res_host_cap < res_bytes) {
        if (rx->res_host) (void)hipHostFree(rx->res_host);   // no copy into it is pending: every plan ends with a synchronisation
        rx->res_host = nullptr;
        rx->res_host_cap = 0;
        LDPC_HIP_TRY(ctx, hipHostMalloc((void **)&rx->res_host, res_bytes, hipHostMallocDefault));
        rx->res_host_cap = res_bytes;
    }
    uint32_t *dense = (uint32_t *)rx->dense.p;
    int32_t *dest = (int32_t *)rx->dest.p, *res = (int32_t *)rx->res.p;
    for (int f = 0; f < nf; f++) {   // (the copy of the previous call's records is behind that call's synchronisation)
        WFlowIn &in = rx->in_host[f];
        in.begin = mixed ? 0 : flow_begin[f]; in.len = mixed ? 0 : flow_begin[f + 1] - flow_begin[f];
        in.base = rx->base[f]; in.ahead = rx->ahead[f];
        for (int j = 0; j < kMaxW; j++) in.cnt[j] = j < W ? rx->cnt[(size_t)f * W + j] : 0;
    }
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(rx->in_dev, rx->in_host, sizeof(WFlowIn) * (size_t)nf, hipMemcpyHostToDevice, ctx->stream));
    // (a) + (b): the plan; a mixed call's on the partition, which also fills in every flow's segment (begin, len) on the device
    const bool aligned4 = plen % 4 == 0 && ((uintptr_t)packets & 3) == 0;
    if (mixed) {
        uint32_t *base = (uint32_t *)res + pl.rec * (size_t)nf, *order = (uint32_t *)rx->order.p;
        if ((rc = demux_launch(ctx, src.flow_of, npackets, nf, base, rx->in_dev, order))) return rc;
        if (aligned4)
            hipLaunchKernelGGL(rxwf_headers_idx<true>, dim3(grid_for(npackets)), dim3(kThreads), 0, ctx->stream, packets, (const uint32_t *)order,
                               (const uint32_t *)base + nf, (int)plen, dense);
        else
            hipLaunchKernelGGL(rxwf_headers_idx<false>, dim3(grid_for(npackets)), dim3(kThreads), 0, ctx->stream, packets, (const uint32_t *)order,
                               (const uint32_t *)base + nf, (int)plen, dense);
        pl.order = order;
        pl.base = (const uint32_t *)rx->res_host + pl.rec * (size_t)nf;
    } else if (aligned4)
        hipLaunchKernelGGL(rxwf_headers<true>, dim3(grid_for(npackets)), dim3(kThreads), 0, ctx->stream, packets, npackets, (int)plen, dense);
    else
        hipLaunchKernelGGL(rxwf_headers<false>, dim3(grid_for(npackets)), dim3(kThreads), 0, ctx->stream, packets, npackets, (int)plen, dense);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    RxwRule r{n, rx->kd, rx->km, W, rx->A};
    if (rx->ruled) {
        const RxwRuleV rv{n, rx->rule.c_hi, rx->rule.later_hi, rx->rule.c_lo, rx->rule.later_lo, W, rx->A};
        if (rx->D > 1)
            hipLaunchKernelGGL(rxw_scan_flows_grouped_ruled, dim3(nf), dim3(64), 0, ctx->stream, (const uint32_t *)dense, (const WFlowIn *)rx->in_dev, rv,
                               rx->D, max_blocks, dest, res);
        else
            hipLaunchKernelGGL(rxw_scan_flows_ruled, dim3(nf), dim3(64), 0, ctx->stream, (const uint32_t *)dense, (const WFlowIn *)rx->in_dev, rv, max_blocks,
                               dest, res);
    } else if (rx->D > 1)
        hipLaunchKernelGGL(rxw_scan_flows_grouped, dim3(nf), dim3(64), 0, ctx->stream, (const uint32_t *)dense, (const WFlowIn *)rx->in_dev, r, rx->D,
                           max_blocks, dest, res);
    else
        hipLaunchKernelGGL(rxw_scan_flows, dim3(nf), dim3(64), 0, ctx->stream, (const uint32_t *)dense, (const WFlowIn *)rx->in_dev, r, max_blocks, dest, res);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(rx->res_host, res, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    LDPC_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = check_device_error(ctx))) return rc;
    int64_t base = 0;
    for (int f = 0; f < nf; f++) {   // the tables of the kernels behind the plan (their copy of the previous call is behind this synchronisation)
        const int32_t *h = rx->res_host + (size_t)f * pl.rec;
        if (h[R_ERR])
            return set_error(ctx, LDPC_AMD_EHIP, "%s: the plan scan of flow %d hit its iteration cap (internal error); every flow's state is unchanged",
                             who, f);
        const int64_t used = word64(h, R_CONSUMED_LO);
        rx->tab_host[f] = WFlowTab{mixed ? (int64_t)pl.base[f] : flow_begin[f], used, (int)base, h[R_CLOSES], rx->head[f], 0};
        base += h[R_CLOSES];
        pl.max_used = std::max(pl.max_used, used);
        if (mixed) pl.max_left = std::max(pl.max_left, (int64_t)(pl.base[f + 1] - pl.base[f]) - used);
    }
    pl.T = (int)base;   // <= nflows * max_blocks < 2^31
    if ((rc = scratch_reserve(ctx, rx->win, sizeof(int32_t) * ((size_t)pl.T + (size_t)W * (size_t)nf) * (size_t)n)) ||
        (rc = scratch_reserve(ctx, rx->slots, sizeof(int32_t) * (size_t)std::max(pl.T, 1))))
        return rc;
    return LDPC_AMD_OK;
}

// the flow table, the slot map and (c): the winners' table of the call, [(T + W nflows)][n]
int rxwf_winners_launch(Rx *rx, const WFlowsPlan &pl)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int nf = rx->nflows;
    int32_t *win = (int32_t *)rx->win.p;
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(rx->tab_dev, rx->tab_host, sizeof(WFlowTab) * (size_t)nf, hipMemcpyHostToDevice, ctx->stream));
    if (pl.T > 0) {
        hipLaunchKernelGGL(rxwf_flow_slots, dim3(nf), dim3(64), 0, ctx->stream, (const WFlowTab *)rx->tab_dev, (int32_t *)rx->slots.p);
        LDPC_HIP_TRY(ctx, hipGetLastError());
    }
    LDPC_HIP_TRY(ctx, hipMemsetAsync(win, 0xff, sizeof(int32_t) * ((size_t)pl.T + (size_t)rx->W * (size_t)nf) * (size_t)rx->n, ctx->stream));   // -1: no packet
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((pl.max_used + kThreads - 1) / kThreads, std::max(1, 32768 / nf)));
    if (pl.order)   // a mixed call planned on positions: the table takes the packet indices
        hipLaunchKernelGGL(rxwf_winners<true>, dim3(gx, nf), dim3(kThreads), 0, ctx->stream, (const uint32_t *)rx->dense.p, (const int32_t *)rx->dest.p,
                           (const WFlowTab *)rx->tab_dev, pl.order, rx->n, rx->W, pl.T, win);
    else
        hipLaunchKernelGGL(rxwf_winners<false>, dim3(gx, nf), dim3(kThreads), 0, ctx->stream, (const uint32_t *)rx->dense.p, (const int32_t *)rx->dest.p,
                           (const WFlowTab *)rx->tab_dev, (const uint32_t *)nullptr, rx->n, rx->W, pl.T, win);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// a mixed call's `left` (may be null): zero, then 1 behind every flow's consumed prefix
int rxwf_left_launch(Rx *rx, const WFlowsPlan &pl, int64_t npackets, uint8_t *left)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (!left) return LDPC_AMD_OK;
    LDPC_HIP_TRY(ctx, hipMemsetAsync(left, 0, (size_t)npackets, ctx->stream));
    if (pl.max_left <= 0) return LDPC_AMD_OK;
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((pl.max_left + kThreads - 1) / kThreads, std::max(1, 32768 / rx->nflows)));
    hipLaunchKernelGGL(rxwf_left, dim3(gx, rx->nflows), dim3(kThreads), 0, ctx->stream, (const WFlowTab *)rx->tab_dev, (const WFlowIn *)rx->in_dev,
                       pl.order, left);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// (d) for the closed slots first .. first + count - 1 (gather) or (e) for the W open blocks of every flow
template <bool GATHER>
int rxwf_move_launch(Rx *rx, const WFlowsPlan &pl, const uint8_t *packets, int first, int count, uint8_t *sym, uint8_t *er)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n, S = rx->S;
    if (GATHER && count <= 0) return LDPC_AMD_OK;
    WFlowMoveArgs a{};
    a.packets = packets; a.plen = (int64_t)S + kHdr; a.win = (const int32_t *)rx->win.p; a.tab = rx->tab_dev;
    a.slot_flow = (const int32_t *)rx->slots.p; a.stage_sym = rx->stage_sym; a.stage_er = rx->stage_er;
    a.sym_out = sym; a.er_out = er; a.n = n; a.S = S; a.W = rx->W; a.T = pl.T; a.nflows = rx->nflows; a.first = first; a.count = count;
    const bool v16 = S % 16 == 0 && ((uintptr_t)packets & 7) == 0 && ((uintptr_t)sym & 15) == 0;
    const int64_t items = (GATHER ? (int64_t)count : (int64_t)rx->W * rx->nflows) * n * (v16 ? S / 16 : S);
    if (v16) hipLaunchKernelGGL((rxwf_move<GATHER, true>), dim3(grid_for(items)), dim3(kThreads), 0, ctx->stream, a);
    else hipLaunchKernelGGL((rxwf_move<GATHER, false>), dim3(grid_for(items)), dim3(kThreads), 0, ctx->stream, a);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// every flow's mirror (base, head, ahead, cnt, totals) and the host outputs: the last step of a call
// (a mixed call: offered and the unrouted count too)
void rxwf_commit(Rx *rx, const WFlowsPlan &pl, int *blocks, int *closes, int64_t *consumed, int64_t npackets, int64_t *offered)
{
    if (pl.base) {
        rx->unrouted += npackets - (int64_t)pl.base[rx->nflows];
        for (int f = 0; offered && f < rx->nflows; f++) offered[f] = (int64_t)(pl.base[f + 1] - pl.base[f]);
    }
    for (int f = 0; f < rx->nflows; f++) {
        const int32_t *h = rx->res_host + (size_t)f * pl.rec;
        const WFlowTab &t = rx->tab_host[f];
        rxw_mirror_commit(rxwf_mirror(rx, f), h, t.closes);
        if (blocks) memcpy(blocks + t.base, h + R_WORDS, sizeof(int) * (size_t)t.closes);
        if (closes) closes[f] = t.closes;
        if (consumed) consumed[f] = t.used;
    }
}

// ---- the flush's plan: the host's, from the mirror (ldpc_amd_fec_rxw_dev_flush per listed flow) -------------------------------------
struct WFlushPlan {
    std::vector<int> sel;          // the listed flows, in list order
    std::vector<int> closes;       // blocks handed out per list entry
    std::vector<int> blocks;       // [T] their wire numbers, in slot order
    std::vector<int32_t> planes;   // [T] their staging planes, f W + b
    int T = 0;
};

int rxwf_flush_plan(const Rx *rx, const char *who, const int32_t *flows, int nsel, WFlushPlan &pl)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (flows) {
        if (nsel < 0 || nsel > rx->nflows) return set_error(ctx, LDPC_AMD_EINVAL, "%s: need 0 <= nsel <= nflows = %d (got %d)", who, rx->nflows, nsel);
        std::vector<uint8_t> seen((size_t)rx->nflows, 0);
        for (int j = 0; j < nsel; j++) {
            const int f = flows[j];
            if (f < 0 || f >= rx->nflows) return set_error(ctx, LDPC_AMD_EINVAL, "%s: no flow %d (nflows = %d)", who, f, rx->nflows);
            if (seen[(size_t)f]) return set_error(ctx, LDPC_AMD_EINVAL, "%s: flow %d is given twice", who, f);
            seen[(size_t)f] = 1;
        }
    } else {
        nsel = rx->nflows;
    }
    pl.sel.resize((size_t)nsel);
    pl.closes.resize((size_t)nsel);
    for (int j = 0; j < nsel; j++) {
        const int f = flows ? flows[j] : j;
        const int count = rxw_mirror_flush_count(&rx->cnt[(size_t)f * rx->W], rx->W);
        pl.sel[(size_t)j] = f;
        pl.closes[(size_t)j] = count;
        for (int c = 0; c < count; c++) {
            pl.blocks.push_back((rx->base[f] + c) & 0xff);
            pl.planes.push_back(f * rx->W + (rx->head[f] + c) % rx->W);
        }
    }
    pl.T = (int)pl.planes.size();   // <= W nflows
    return LDPC_AMD_OK;
}

// COPY: slots first .. first + count - 1 -> sym / er, their planes reset in the same launch; else: the planes of those slots reset
template <bool COPY>
int rxwf_flush_launch(Rx *rx, int first, int count, uint8_t *sym, uint8_t *er)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n, S = rx->S;
    const bool v16 = S % 16 == 0 && ((uintptr_t)sym & 15) == 0;
    const int64_t pieces = (int64_t)n * (v16 ? S / 16 : S);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((pieces + kThreads - 1) / kThreads, 256)), (unsigned)std::min(count, 16384));
    if (v16) hipLaunchKernelGGL((rxwf_flush_move<16, COPY>), grid, dim3(kThreads), 0, ctx->stream, (const int32_t *)rx->fl.dev, rx->stage_sym, rx->stage_er, n, S, first, count, sym, er);
    else hipLaunchKernelGGL((rxwf_flush_move<1, COPY>), grid, dim3(kThreads), 0, ctx->stream, (const int32_t *)rx->fl.dev, rx->stage_sym, rx->stage_er, n, S, first, count, sym, er);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// the mirror of every listed flow after its flush -- each handed-out block a close -- and the host outputs
void rxwf_flush_commit(Rx *rx, const WFlushPlan &pl, int *blocks, int *closes)
{
    for (size_t j = 0; j < pl.sel.size(); j++) {
        if (closes) closes[j] = pl.closes[j];
        if (pl.closes[j] > 0) rxw_mirror_flush(rxwf_mirror(rx, pl.sel[j]), pl.closes[j], nullptr);
    }
    if (blocks && pl.T > 0) memcpy(blocks, pl.blocks.data(), sizeof(int) * (size_t)pl.T);
}

}  // namespace

extern "C" {

int ldpc_amd_fec_rxw_flows_create(ldpc_amd_ctx *ctx, int nflows, int n, int k, int S, int window, int ahead_limit, ldpc_amd_fec_rxw_flows **out)
{
    return ldpc_amd_fec_rxw_flows_create_rule(ctx, nflows, n, k, S, window, ahead_limit, 1, nullptr, out);
}

int ldpc_amd_fec_rxw_flows_depth(const ldpc_amd_fec_rxw_flows *rx) { return rx ? rx->D : -1; }

int ldpc_amd_fec_rxw_flows_get_rule(const ldpc_amd_fec_rxw_flows *rx, ldpc_amd_fec_rx_rule *rule)
{
    if (!rx || !rule) return LDPC_AMD_EINVAL;
    *rule = rx->rule;
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_rxw_flows_create_depth(ldpc_amd_ctx *ctx, int nflows, int n, int k, int S, int window, int ahead_limit, int depth,
                                        ldpc_amd_fec_rxw_flows **out)
{
    return ldpc_amd_fec_rxw_flows_create_rule(ctx, nflows, n, k, S, window, ahead_limit, depth, nullptr, out);
}

int ldpc_amd_fec_rxw_flows_create_rule(ldpc_amd_ctx *ctx, int nflows, int n, int k, int S, int window, int ahead_limit, int depth,
                                       const ldpc_amd_fec_rx_rule *rule, ldpc_amd_fec_rxw_flows **out)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!out || nflows < 1 || nflows > kMaxFlows || n <= 0 || n > 65536 || k <= 0 || k >= n || S <= 0)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_flows_create: need 1 <= nflows <= 4096, n <= 65536, 0 < k < n, S >= 1 (nflows=%d n=%d k=%d S=%d)",
                         nflows, n, k, S);
    int rc;
    if ((rc = rxw_check_create(ctx, "fec_rxw_flows_create", window, ahead_limit, (int64_t)nflows * window * n, "nflows * window * n"))) return rc;
    if (!LDPC_AMD_FEC_ILV_DEPTH_OK(depth) || (depth > 1 && 2 * depth > window))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_flows_create: depth must be 1, 2, 4, 8 or 16, and a depth > 1 needs 2 * depth <= window (depth=%d window=%d)",
                         depth, window);
    ldpc_amd_fec_rx_rule rl{};
    bool ruled = false;
    if (rxw_rule_resolve(n, k, rule, &rl, &ruled))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_flows_create: invalid close rule (%d, %d, %d, %d): need 0 <= c <= n = %d, 0 <= later <= 2^30, and later >= 1 where c == 0",
                         rl.c_hi, rl.later_hi, rl.c_lo, rl.later_lo, n);
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    Rx *rx = new (std::nothrow) Rx();
    if (!rx) return set_error(ctx, LDPC_AMD_ENOMEM, "fec_rxw_flows_create: out of host memory");
    rx->ctx = ctx;
    rx->nflows = nflows; rx->n = n; rx->k = k; rx->S = S; rx->W = window; rx->A = ahead_limit; rx->D = depth;
    rx->rule = rl; rx->ruled = ruled;
    rx->kd = k + (int)lround((n - k) * 0.8);
    rx->km = k + (int)lround((n - k) * 0.2);
    rx->base.assign((size_t)nflows, -1); rx->head.assign((size_t)nflows, 0); rx->ahead.assign((size_t)nflows, 0);
    rx->cnt.assign((size_t)nflows * window, 0);
    rx->totals.assign((size_t)nflows * 5, 0);
    const size_t planes = (size_t)nflows * window, plane = (size_t)n * S;
    // (a request beyond the device's memory is not always answered with hipErrorOutOfMemory: a staging plane that cannot be had is ENOMEM)
    hipError_t e = hipMalloc((void **)&rx->stage_sym, planes * plane);
    if (e == hipSuccess) e = hipMalloc((void **)&rx->stage_er, planes * (size_t)n);
    const bool no_planes = e != hipSuccess;
    if (e == hipSuccess) e = hipMalloc((void **)&rx->in_dev, sizeof(WFlowIn) * (size_t)nflows);
    if (e == hipSuccess) e = hipMalloc((void **)&rx->tab_dev, sizeof(WFlowTab) * (size_t)nflows);
    if (e == hipSuccess) e = hipHostMalloc((void **)&rx->in_host, sizeof(WFlowIn) * (size_t)nflows, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&rx->tab_host, sizeof(WFlowTab) * (size_t)nflows, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(rx->stage_sym, 0, planes * plane, ctx->stream);   // payload zero, every symbol erased
    if (e == hipSuccess) e = hipMemsetAsync(rx->stage_er, 1, planes * (size_t)n, ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ldpc_amd_fec_rxw_flows_destroy(rx);
        return set_error(ctx, no_planes || e == hipErrorOutOfMemory ? LDPC_AMD_ENOMEM : LDPC_AMD_EHIP, "fec_rxw_flows_create: %s%s",
                         no_planes ? "the staging planes do not fit: " : "", hipGetErrorString(e));
    }
    *out = rx;
    return LDPC_AMD_OK;
}

void ldpc_amd_fec_rxw_flows_destroy(ldpc_amd_fec_rxw_flows *rx)
{
    if (!rx) return;
    (void)hipSetDevice(rx->ctx->device);
    (void)hipStreamSynchronize(rx->ctx->stream);   // pending work of this object may still use its buffers
    Scratch *sc[] = {&rx->dense, &rx->dest, &rx->win, &rx->res, &rx->slots, &rx->order};
    for (Scratch *s : sc)
        if (s->p) (void)hipFree(s->p);
    void *dev[] = {rx->stage_sym, rx->stage_er, rx->in_dev, rx->tab_dev};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    void *host[] = {rx->in_host, rx->tab_host, rx->res_host};
    for (void *p : host)
        if (p) (void)hipHostFree(p);
    rx_upload_free(rx->fl);
    delete rx;
}

int ldpc_amd_fec_rxw_flows_stats(const ldpc_amd_fec_rxw_flows *rx, int flow, int64_t totals[5])
{
    if (!rx || !totals || flow < 0 || flow >= rx->nflows) return LDPC_AMD_EINVAL;
    memcpy(totals, &rx->totals[(size_t)flow * 5], sizeof(int64_t) * 5);
    return LDPC_AMD_OK;
}

int64_t ldpc_amd_fec_rxw_flows_dropped(const ldpc_amd_fec_rxw_flows *rx, int flow)
{
    if (!rx || flow < 0 || flow >= rx->nflows) return -1;
    const int64_t *t = &rx->totals[(size_t)flow * 5];
    return t[LDPC_AMD_RXW_BAD_SYMBOL] + t[LDPC_AMD_RXW_LATE] + t[LDPC_AMD_RXW_AHEAD];
}

int ldpc_amd_fec_rxw_flows_state(const ldpc_amd_fec_rxw_flows *rx, int flow, int *base, int *cnt, int64_t *ahead)
{
    if (!rx || flow < 0 || flow >= rx->nflows) return LDPC_AMD_EINVAL;
    if (base) *base = rx->base[flow];
    if (cnt) memcpy(cnt, &rx->cnt[(size_t)flow * rx->W], sizeof(int) * (size_t)rx->W);
    if (ahead) *ahead = rx->ahead[flow];
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_rxw_flows_pending(const ldpc_amd_fec_rxw_flows *rx, int32_t *base, int32_t *cnt)
{
    if (!rx) return LDPC_AMD_EINVAL;
    int total = 0;
    for (int f = 0; f < rx->nflows; f++) {
        if (base) base[f] = rx->base[f];
        total += rxw_mirror_flush_count(&rx->cnt[(size_t)f * rx->W], rx->W);
    }
    if (cnt) memcpy(cnt, rx->cnt.data(), sizeof(int32_t) * rx->cnt.size());
    return total;
}

}  // extern "C"

namespace {

// push_many and push_mixed: P is the segmented call's flow_begin[nflows], or the mixed call's argument
int rxwf_push(Rx *rx, const char *who, const uint8_t *packets, const WFlowsSrc &src, int64_t P, uint8_t *sym_batch, uint8_t *erased_batch,
              int *blocks, int *closes, int max_blocks_per_flow, int64_t *consumed, int64_t *offered, uint8_t *left)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    const bool mixed = src.mixed;
    int rc;
    if ((rc = mixed ? rxwf_check_limits(rx, who, P, max_blocks_per_flow) : rxwf_check_call(rx, who, src.flow_begin, max_blocks_per_flow, P)))
        return rc;
    if (!sym_batch || !erased_batch || (P > 0 && !packets))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: packets / sym_batch / erased_batch must not be null", who);
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((P > 0 && !is_device_ptr(ctx, packets)) || !is_device_ptr(ctx, sym_batch) || !is_device_ptr(ctx, erased_batch))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: packets / sym_batch / erased_batch must be device pointers of device %d", who, ctx->device);
    if (P == 0) {
        rxwf_nothing(rx, closes, consumed, offered);
        return 0;
    }
    if (mixed && (rc = rxwf_check_mixed(rx, who, src.flow_of, left))) return rc;
    WFlowsPlan pl;
    if ((rc = rxwf_plan(rx, who, packets, src, P, max_blocks_per_flow, pl))) return rc;
    // (c), (d), (e): the data movement, asynchronous
    if ((rc = rxwf_winners_launch(rx, pl)) || (rc = rxwf_move_launch<true>(rx, pl, packets, 0, pl.T, sym_batch, erased_batch)) ||
        (rc = rxwf_move_launch<false>(rx, pl, packets, 0, 0, sym_batch, nullptr)) || (rc = rxwf_left_launch(rx, pl, P, left)))
        return rc;
    rxwf_commit(rx, pl, blocks, closes, consumed, P, offered);
    return pl.T;
}

// push_many + decode_frames in one call (rx_host.h: the decode driver).  FUSED where the decoder can fetch its rows from the packets
// itself (decode_reads_packets): (d) shrinks to rxwf_sources, the planes of all flows being one `stage` base.  Else COMPOSED: (d)
// gathers chunk by chunk.  (e) is launched BEHIND the decode in both forms: it overwrites the staging planes of the carried blocks,
// which the fused decode reads.
int rxwf_decode(Rx *rx, const char *who, int code, const uint8_t *packets, const WFlowsSrc &src, int64_t P, int max_sweeps, int do_ml, uint8_t *out,
                int32_t *sweeps, int32_t *residual, int32_t *status, uint8_t *erased_out, int32_t *residual_src, int *blocks, int *closes,
                int max_blocks_per_flow, int64_t *consumed, int64_t *offered, uint8_t *left)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    if (code < 0 || code >= (int)ctx->codes.size()) return set_error(ctx, LDPC_AMD_ENOCODE, "unknown code handle %d", code);
    const bool mixed = src.mixed;
    int rc;
    if ((rc = mixed ? rxwf_check_limits(rx, who, P, max_blocks_per_flow) : rxwf_check_call(rx, who, src.flow_begin, max_blocks_per_flow, P)))
        return rc;
    if (P == 0) {
        rxwf_nothing(rx, closes, consumed, offered);
        return 0;
    }
    const RxResults o{out, sweeps, residual, status, erased_out, residual_src};
    if ((rc = rx_decode_check(ctx, rx, who, code, max_sweeps, o))) return rc;
    if (!packets || !is_device_ptr(ctx, packets))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: packets must be a device pointer of device %d", who, ctx->device);
    if (mixed && (rc = rxwf_check_mixed(rx, who, src.flow_of, left))) return rc;
    const DevCode &cd = ctx->codes[code]->dev;
    const int n = rx->n, S = rx->S;
    const bool fused = ctx->knobs.rx_pkt != 0 && ((uintptr_t)packets & 7) == 0 && decode_reads_packets(ctx, cd, S);
    const size_t frame = (size_t)n * S;

    WFlowsPlan pl;
    if ((rc = rxwf_plan(rx, who, packets, src, P, max_blocks_per_flow, pl))) return rc;
    const int T = pl.T;
    const int64_t chunk = rx_chunk(T, frame);
    size_t scratch = 0;
    if ((rc = rx_decode_reserve(ctx, T, n, frame, fused, chunk, &scratch))) return rc;
    if ((rc = rxwf_winners_launch(rx, pl))) return rc;
    DecodeArgs d = rx_decode_args(cd, n, S, max_sweeps, do_ml);
    const PacketRows pin{nullptr, packets, rx->stage_sym, S + kHdr};
    auto sources = [&](uint32_t *src, uint8_t *er) -> int {
        hipLaunchKernelGGL(rxwf_sources, dim3(grid_for((int64_t)T * n)), dim3(kThreads), 0, ctx->stream, (const int32_t *)rx->win.p,
                           (const uint8_t *)rx->stage_er, (const WFlowTab *)rx->tab_dev, (const int32_t *)rx->slots.p, n, rx->W, T, src, er);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        return LDPC_AMD_OK;
    };
    auto gather = [&](int first, int count, uint8_t *sym, uint8_t *er) { return rxwf_move_launch<true>(rx, pl, packets, first, count, sym, er); };
    int launches = 0;
    if ((rc = rx_decode_slots(ctx, d, o, T, chunk, fused, pin, sources, gather, &launches))) return rc;
    if ((rc = rxwf_move_launch<false>(rx, pl, packets, 0, 0, nullptr, nullptr))) return rc;   // (e)
    if ((rc = rxwf_left_launch(rx, pl, P, left))) return rc;
    rxwf_commit(rx, pl, blocks, closes, consumed, P, offered);
    ctx->rxwf_info[0] = fused ? 1 : 2; ctx->rxwf_info[1] = T; ctx->rxwf_info[2] = launches; ctx->rxwf_info[3] = (int64_t)scratch;
    return T;
}

}  // namespace

extern "C" {

int ldpc_amd_fec_rxw_flows_push_many(ldpc_amd_fec_rxw_flows *rx, const uint8_t *packets, const int64_t *flow_begin, uint8_t *sym_batch,
                                     uint8_t *erased_batch, int *blocks, int *closes, int max_blocks_per_flow, int64_t *consumed)
{
    WFlowsSrc src;
    src.flow_begin = flow_begin;
    return rxwf_push(rx, "fec_rxw_flows_push_many", packets, src, 0, sym_batch, erased_batch, blocks, closes, max_blocks_per_flow, consumed, nullptr,
                     nullptr);
}

int ldpc_amd_fec_rxw_flows_decode_many(ldpc_amd_fec_rxw_flows *rx, int code, const uint8_t *packets, const int64_t *flow_begin, int max_sweeps,
                                       int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status, uint8_t *erased_out,
                                       int32_t *residual_src, int *blocks, int *closes, int max_blocks_per_flow, int64_t *consumed)
{
    WFlowsSrc src;
    src.flow_begin = flow_begin;
    return rxwf_decode(rx, "fec_rxw_flows_decode_many", code, packets, src, 0, max_sweeps, do_ml, out, sweeps, residual, status, erased_out,
                       residual_src, blocks, closes, max_blocks_per_flow, consumed, nullptr, nullptr);
}

// ---- interleaved packets (include/ldpc_erasure_amd_rx_window_flows_mixed.h) ---------------------------------------------------------
int ldpc_amd_fec_rxw_flows_push_mixed(ldpc_amd_fec_rxw_flows *rx, const uint8_t *packets, const int32_t *flow_of, int64_t P, uint8_t *sym_batch,
                                      uint8_t *erased_batch, int *blocks, int *closes, int max_blocks_per_flow, int64_t *consumed,
                                      int64_t *offered, uint8_t *left)
{
    WFlowsSrc src;
    src.mixed = true;
    src.flow_of = flow_of;
    return rxwf_push(rx, "fec_rxw_flows_push_mixed", packets, src, P, sym_batch, erased_batch, blocks, closes, max_blocks_per_flow, consumed, offered,
                     left);
}

int ldpc_amd_fec_rxw_flows_decode_mixed(ldpc_amd_fec_rxw_flows *rx, int code, const uint8_t *packets, const int32_t *flow_of, int64_t P,
                                        int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                        uint8_t *erased_out, int32_t *residual_src, int *blocks, int *closes, int max_blocks_per_flow,
                                        int64_t *consumed, int64_t *offered, uint8_t *left)
{
    WFlowsSrc src;
    src.mixed = true;
    src.flow_of = flow_of;
    return rxwf_decode(rx, "fec_rxw_flows_decode_mixed", code, packets, src, P, max_sweeps, do_ml, out, sweeps, residual, status, erased_out,
                       residual_src, blocks, closes, max_blocks_per_flow, consumed, offered, left);
}

int64_t ldpc_amd_fec_rxw_flows_unrouted(const ldpc_amd_fec_rxw_flows *rx) { return rx ? rx->unrouted : -1; }

int ldpc_amd_fec_rxw_flows_flush_many(ldpc_amd_fec_rxw_flows *rx, const int32_t *flows, int nsel, uint8_t *sym_batch, uint8_t *erased_batch,
                                      int *blocks, int *closes)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    const char *who = "fec_rxw_flows_flush_many";
    WFlushPlan pl;
    int rc;
    if ((rc = rxwf_flush_plan(rx, who, flows, nsel, pl))) return rc;
    if (!sym_batch || !erased_batch) return set_error(ctx, LDPC_AMD_EINVAL, "%s: sym_batch / erased_batch must not be null", who);
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!is_device_ptr(ctx, sym_batch) || !is_device_ptr(ctx, erased_batch))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: sym_batch / erased_batch must be device pointers of device %d", who, ctx->device);
    if (pl.T == 0) {
        if (closes) std::fill(closes, closes + pl.sel.size(), 0);
        return 0;
    }
    if ((rc = rx_upload_planes(ctx, who, rx->fl, (size_t)rx->W * (size_t)rx->nflows, pl.planes.data(), pl.T)) ||
        (rc = rxwf_flush_launch<true>(rx, 0, pl.T, sym_batch, erased_batch)))
        return rc;
    rxwf_flush_commit(rx, pl, blocks, closes);
    return pl.T;
}

// flush_many + decode.  FUSED where the decoder has the packets-in form and S % 16 == 0: every row of every block is staged (or erased),
// rxwf_flush_sources names it and ONE launch_decode follows the words into the planes; the planes are reset by one launch behind it.
// Else COMPOSED: a chunk of planes goes to the scratch (and is reset in the same launch) and through the decoder.
int ldpc_amd_fec_rxw_flows_decode_flush_many(ldpc_amd_fec_rxw_flows *rx, int code, const int32_t *flows, int nsel, int max_sweeps, int do_ml,
                                             uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status, uint8_t *erased_out,
                                             int32_t *residual_src, int *blocks, int *closes)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    const char *who = "fec_rxw_flows_decode_flush_many";
    WFlushPlan pl;
    int rc;
    if ((rc = rxwf_flush_plan(rx, who, flows, nsel, pl))) return rc;
    const RxResults o{out, sweeps, residual, status, erased_out, residual_src};
    if ((rc = rx_decode_check(ctx, rx, who, code, max_sweeps, o))) return rc;
    const int T = pl.T;
    if (T == 0) {
        if (closes) std::fill(closes, closes + pl.sel.size(), 0);
        return 0;
    }
    const DevCode &cd = ctx->codes[code]->dev;
    const int n = rx->n, S = rx->S;
    const bool fused = ctx->knobs.rx_pkt != 0 && S % 16 == 0 && decode_reads_packets(ctx, cd, S);
    const size_t frame = (size_t)n * S;
    const int64_t chunk = rx_chunk(T, frame);
    size_t scratch = 0;
    if ((rc = rx_decode_reserve(ctx, T, n, frame, fused, chunk, &scratch))) return rc;
    if ((rc = rx_upload_planes(ctx, who, rx->fl, (size_t)rx->W * (size_t)rx->nflows, pl.planes.data(), pl.T))) return rc;
    DecodeArgs d = rx_decode_args(cd, n, S, max_sweeps, do_ml);
    // no word of the table names a packet (rxwf_flush_sources), so the packet base is never added to: any valid aligned address
    const PacketRows pin{nullptr, rx->stage_sym, rx->stage_sym, S + kHdr};
    auto sources = [&](uint32_t *src, uint8_t *er) -> int {
        hipLaunchKernelGGL(rxwf_flush_sources, dim3(grid_for((int64_t)T * n)), dim3(kThreads), 0, ctx->stream, (const int32_t *)rx->fl.dev,
                           (const uint8_t *)rx->stage_er, n, T, src, er);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        return LDPC_AMD_OK;
    };
    // (composed: a chunk's planes are reset by the launch that copies them)
    auto gather = [&](int first, int count, uint8_t *sym, uint8_t *er) { return rxwf_flush_launch<true>(rx, first, count, sym, er); };
    int launches = 0;
    if ((rc = rx_decode_slots(ctx, d, o, T, chunk, fused, pin, sources, gather, &launches))) return rc;
    if (fused && (rc = rxwf_flush_launch<false>(rx, 0, T, nullptr, nullptr))) return rc;   // the planes reset, behind the decode that reads them
    rxwf_flush_commit(rx, pl, blocks, closes);
    ctx->rxwf_info[0] = fused ? 1 : 2; ctx->rxwf_info[1] = T; ctx->rxwf_info[2] = launches; ctx->rxwf_info[3] = (int64_t)scratch;
    return T;
}

int ldpc_amd_fec_rxw_flows_info(ldpc_amd_ctx *ctx, int64_t info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_flows_info: info must not be null");
    memcpy(info, ctx->rxwf_info, sizeof(ctx->rxwf_info));
    return LDPC_AMD_OK;
}

}  // extern "C"
