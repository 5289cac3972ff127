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
// flow's window, the upload of the flush's plane numbers -- is csrc/rx_host.h.  The calls themselves -- checks, plan, push, decode,
// commit, batch flush, create and destroy -- are csrc/rx_flows_host.h's, shared with wire_dev.hip's flows; this unit gives it the
// kernels and the window's rules as WFlowsPolicy.
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
#include "rx_flows_host.h"   // the multi-flow call skeleton; with it rx_host.h, rx_window_scan_dev.h and flows_demux_dev.h (kMaxFlows)

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

inline RxwMirror rxwf_mirror(Rx *rx, int f)
{
    return RxwMirror{&rx->base[f], &rx->head[f], &rx->ahead[f], &rx->cnt[(size_t)f * rx->W], &rx->totals[(size_t)f * 5], rx->W};
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

// What the windowed receiver puts into the multi-flow call skeleton (rx_flows_host.h)
struct WFlowsPolicy {
    typedef ldpc_amd_fec_rxw_flows Rx;
    static int planes_per_flow(const Rx *rx) { return rx->W; }
    static void fill_in(Rx *rx, int f, int64_t begin, int64_t len)
    {
        WFlowIn &in = rx->in_host[f];
        in.begin = begin; in.len = len;
        in.base = rx->base[f]; in.ahead = rx->ahead[f];
        for (int j = 0; j < kMaxW; j++) in.cnt[j] = j < rx->W ? rx->cnt[(size_t)f * rx->W + j] : 0;
    }
    static int launch_headers(Rx *rx, bool aligned4, const uint8_t *packets, const int32_t *flow_of, uint32_t *base, uint32_t *order, int64_t np,
                              int plen, uint32_t *dense)
    {
        hipStream_t st = rx->ctx->stream;
        const int nf = rx->nflows;
        int rc;
        if (order && (rc = demux_launch(rx->ctx, flow_of, np, nf, base, rx->in_dev, order))) return rc;
        const uint32_t *ord = order, *routed = order ? base + nf : nullptr;   // the routed count, as the partition's bases kernel wrote it
        if (order && aligned4) hipLaunchKernelGGL(rxwf_headers_idx<true>, dim3(grid_for(np)), dim3(kThreads), 0, st, packets, ord, routed, plen, dense);
        else if (order) hipLaunchKernelGGL(rxwf_headers_idx<false>, dim3(grid_for(np)), dim3(kThreads), 0, st, packets, ord, routed, plen, dense);
        else if (aligned4) hipLaunchKernelGGL(rxwf_headers<true>, dim3(grid_for(np)), dim3(kThreads), 0, st, packets, np, plen, dense);
        else hipLaunchKernelGGL(rxwf_headers<false>, dim3(grid_for(np)), dim3(kThreads), 0, st, packets, np, plen, dense);
        return LDPC_AMD_OK;
    }
    // the only step that looks at the depth and at the rule
    static void launch_scan(Rx *rx, const uint32_t *dense, int max_blocks, int32_t *dest, int32_t *res)
    {
        hipStream_t st = rx->ctx->stream;
        const int nf = rx->nflows, n = rx->n, W = rx->W;
        const WFlowIn *in = rx->in_dev;
        RxwRule r{n, rx->kd, rx->km, W, rx->A};
        if (rx->ruled) {
            const RxwRuleV rv{n, rx->rule.c_hi, rx->rule.later_hi, rx->rule.c_lo, rx->rule.later_lo, W, rx->A};
            if (rx->D > 1) hipLaunchKernelGGL(rxw_scan_flows_grouped_ruled, dim3(nf), dim3(64), 0, st, dense, in, rv, rx->D, max_blocks, dest, res);
            else hipLaunchKernelGGL(rxw_scan_flows_ruled, dim3(nf), dim3(64), 0, st, dense, in, rv, max_blocks, dest, res);
        } else if (rx->D > 1)
            hipLaunchKernelGGL(rxw_scan_flows_grouped, dim3(nf), dim3(64), 0, st, dense, in, r, rx->D, max_blocks, dest, res);
        else
            hipLaunchKernelGGL(rxw_scan_flows, dim3(nf), dim3(64), 0, st, dense, in, r, max_blocks, dest, res);
    }
    static size_t rec_words(int max_blocks) { return (size_t)R_WORDS + (size_t)max_blocks; }
    static bool err(const int32_t *h) { return h[R_ERR] != 0; }
    static int closes(const int32_t *h) { return h[R_CLOSES]; }
    static int64_t consumed(const int32_t *h) { return word64(h, R_CONSUMED_LO); }
    static WFlowTab tab_entry(const Rx *rx, int f, int64_t begin, int64_t used, int base, int closes)
    {
        return WFlowTab{begin, used, base, closes, rx->head[f], 0};
    }
    static void launch_slots(Rx *rx)
    {
        hipLaunchKernelGGL(rxwf_flow_slots, dim3(rx->nflows), dim3(64), 0, rx->ctx->stream, (const WFlowTab *)rx->tab_dev, (int32_t *)rx->slots.p);
    }
    // a mixed call planned on positions: the table takes the packet indices
    static int launch_winners(Rx *rx, const RxFlowsPlan &pl, unsigned gx, int32_t *win)
    {
        ldpc_amd_ctx *ctx = rx->ctx;
        if (pl.order)
            hipLaunchKernelGGL(rxwf_winners<true>, dim3(gx, rx->nflows), dim3(kThreads), 0, ctx->stream, (const uint32_t *)rx->dense.p,
                               (const int32_t *)rx->dest.p, (const WFlowTab *)rx->tab_dev, pl.order, rx->n, rx->W, pl.T, win);
        else
            hipLaunchKernelGGL(rxwf_winners<false>, dim3(gx, rx->nflows), dim3(kThreads), 0, ctx->stream, (const uint32_t *)rx->dense.p,
                               (const int32_t *)rx->dest.p, (const WFlowTab *)rx->tab_dev, (const uint32_t *)nullptr, rx->n, rx->W, pl.T, win);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        return LDPC_AMD_OK;
    }
    static void launch_left(Rx *rx, const RxFlowsPlan &pl, unsigned gx, uint8_t *left)
    {
        hipLaunchKernelGGL(rxwf_left, dim3(gx, rx->nflows), dim3(kThreads), 0, rx->ctx->stream, (const WFlowTab *)rx->tab_dev,
                           (const WFlowIn *)rx->in_dev, pl.order, left);
    }
    static void launch_move(Rx *rx, const RxFlowsPlan &pl, const uint8_t *packets, bool gather, int first, int count, uint8_t *sym, uint8_t *er,
                            bool v16, int64_t items)
    {
        WFlowMoveArgs a{};
        a.packets = packets; a.plen = (int64_t)rx->S + kHdr; a.win = (const int32_t *)rx->win.p; a.tab = rx->tab_dev;
        a.slot_flow = (const int32_t *)rx->slots.p; a.stage_sym = rx->stage_sym; a.stage_er = rx->stage_er;
        a.sym_out = sym; a.er_out = er; a.n = rx->n; a.S = rx->S; a.W = rx->W; a.T = pl.T; a.nflows = rx->nflows; a.first = first; a.count = count;
        const dim3 grid(grid_for(items)), block(kThreads);
        hipStream_t st = rx->ctx->stream;
        if (gather && v16) hipLaunchKernelGGL((rxwf_move<true, true>), grid, block, 0, st, a);
        else if (gather) hipLaunchKernelGGL((rxwf_move<true, false>), grid, block, 0, st, a);
        else if (v16) hipLaunchKernelGGL((rxwf_move<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((rxwf_move<false, false>), grid, block, 0, st, a);
    }
    static void launch_sources(Rx *rx, int T, uint32_t *src, uint8_t *er)
    {
        hipLaunchKernelGGL(rxwf_sources, dim3(grid_for((int64_t)T * rx->n)), dim3(kThreads), 0, rx->ctx->stream, (const int32_t *)rx->win.p,
                           (const uint8_t *)rx->stage_er, (const WFlowTab *)rx->tab_dev, (const int32_t *)rx->slots.p, rx->n, rx->W, T, src, er);
    }
    static void commit_flow(Rx *rx, int f, const int32_t *h, int closes) { rxw_mirror_commit(rxwf_mirror(rx, f), h, closes); }
    static void record_info(ldpc_amd_ctx *ctx, bool fused, int T, int launches, size_t scratch)
    {
        ctx->rxwf_info[0] = fused ? 1 : 2; ctx->rxwf_info[1] = T; ctx->rxwf_info[2] = launches; ctx->rxwf_info[3] = (int64_t)scratch;
    }
    // ---- the flush (ldpc_amd_fec_rxw_dev_flush per listed flow): every open slot up to the last non-empty one ----
    static int flush_fill(const Rx *rx, int f, int, RxFlushPlan &pl)
    {
        const int count = rxw_mirror_flush_count(&rx->cnt[(size_t)f * rx->W], rx->W);
        for (int c = 0; c < count; c++) {
            pl.blocks.push_back((rx->base[f] + c) & 0xff);
            pl.planes.push_back(f * rx->W + (rx->head[f] + c) % rx->W);
        }
        return count;
    }
    // (a chunk's planes are reset by the launch that copies them; the fused decode reads them, so their reset stands behind it)
    static int flush_gather(Rx *rx, int first, int count, uint8_t *sym, uint8_t *er) { return rxwf_flush_launch<true>(rx, first, count, sym, er); }
    static int flush_after(Rx *rx, bool fused, int T) { return fused ? rxwf_flush_launch<false>(rx, 0, T, nullptr, nullptr) : LDPC_AMD_OK; }
    static void launch_flush_sources(Rx *rx, int T, uint32_t *src, uint8_t *er)
    {
        hipLaunchKernelGGL(rxwf_flush_sources, dim3(grid_for((int64_t)T * rx->n)), dim3(kThreads), 0, rx->ctx->stream, (const int32_t *)rx->fl.dev,
                           (const uint8_t *)rx->stage_er, rx->n, T, src, er);
    }
    static void flush_commit_flow(Rx *rx, int f, int count)   // each handed-out block a close
    {
        if (count > 0) rxw_mirror_flush(rxwf_mirror(rx, f), count, nullptr);
    }
    static void record_flush(ldpc_amd_ctx *ctx, int path, int T, int, int launches, size_t scratch)   // (flush_many writes no info word)
    {
        if (path != 3) record_info(ctx, path == 1, T, launches, scratch);
    }
};
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
    return rxf_create_buffers<WFlowsPolicy>(ctx, rx, "fec_rxw_flows_create", out);
}

void ldpc_amd_fec_rxw_flows_destroy(ldpc_amd_fec_rxw_flows *rx) { rxf_destroy(rx); }

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

// ---- the calls: each fills in where its packets are and runs the skeleton (rx_flows_host.h) under its own name ----------------------
int ldpc_amd_fec_rxw_flows_push_many(ldpc_amd_fec_rxw_flows *rx, const uint8_t *packets, const int64_t *flow_begin, uint8_t *sym_batch,
                                     uint8_t *erased_batch, int *blocks, int *closes, int max_blocks_per_flow, int64_t *consumed)
{
    return rxf_push<WFlowsPolicy>(rx, "fec_rxw_flows_push_many", packets, RxFlowsSrc{false, flow_begin, nullptr}, 0, sym_batch, erased_batch,
                                  max_blocks_per_flow, RxFlowsOut{blocks, closes, consumed, nullptr, nullptr});
}

int ldpc_amd_fec_rxw_flows_decode_many(ldpc_amd_fec_rxw_flows *rx, int code, const uint8_t *packets, const int64_t *flow_begin, int max_sweeps,
                                       int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status, uint8_t *erased_out,
                                       int32_t *residual_src, int *blocks, int *closes, int max_blocks_per_flow, int64_t *consumed)
{
    return rxf_decode<WFlowsPolicy>(rx, "fec_rxw_flows_decode_many", code, packets, RxFlowsSrc{false, flow_begin, nullptr}, 0, max_sweeps, do_ml,
                                    RxResults{out, sweeps, residual, status, erased_out, residual_src}, max_blocks_per_flow,
                                    RxFlowsOut{blocks, closes, consumed, nullptr, nullptr});
}

// interleaved packets (include/ldpc_erasure_amd_rx_window_flows_mixed.h)
int ldpc_amd_fec_rxw_flows_push_mixed(ldpc_amd_fec_rxw_flows *rx, const uint8_t *packets, const int32_t *flow_of, int64_t P, uint8_t *sym_batch,
                                      uint8_t *erased_batch, int *blocks, int *closes, int max_blocks_per_flow, int64_t *consumed,
                                      int64_t *offered, uint8_t *left)
{
    return rxf_push<WFlowsPolicy>(rx, "fec_rxw_flows_push_mixed", packets, RxFlowsSrc{true, nullptr, flow_of}, P, sym_batch, erased_batch,
                                  max_blocks_per_flow, RxFlowsOut{blocks, closes, consumed, offered, left});
}

int ldpc_amd_fec_rxw_flows_decode_mixed(ldpc_amd_fec_rxw_flows *rx, int code, const uint8_t *packets, const int32_t *flow_of, int64_t P,
                                        int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                        uint8_t *erased_out, int32_t *residual_src, int *blocks, int *closes, int max_blocks_per_flow,
                                        int64_t *consumed, int64_t *offered, uint8_t *left)
{
    return rxf_decode<WFlowsPolicy>(rx, "fec_rxw_flows_decode_mixed", code, packets, RxFlowsSrc{true, nullptr, flow_of}, P, max_sweeps, do_ml,
                                    RxResults{out, sweeps, residual, status, erased_out, residual_src}, max_blocks_per_flow,
                                    RxFlowsOut{blocks, closes, consumed, offered, left});
}

int64_t ldpc_amd_fec_rxw_flows_unrouted(const ldpc_amd_fec_rxw_flows *rx) { return rx ? rx->unrouted : -1; }

int ldpc_amd_fec_rxw_flows_flush_many(ldpc_amd_fec_rxw_flows *rx, const int32_t *flows, int nsel, uint8_t *sym_batch, uint8_t *erased_batch,
                                      int *blocks, int *closes)
{
    if (!rx) return LDPC_AMD_EINVAL;
    return rxf_flush_many<WFlowsPolicy>(rx, "fec_rxw_flows_flush_many", flows, nsel, 0, sym_batch, erased_batch, blocks, closes);
}

int ldpc_amd_fec_rxw_flows_decode_flush_many(ldpc_amd_fec_rxw_flows *rx, int code, const int32_t *flows, int nsel, int max_sweeps, int do_ml,
                                             uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status, uint8_t *erased_out,
                                             int32_t *residual_src, int *blocks, int *closes)
{
    if (!rx) return LDPC_AMD_EINVAL;
    return rxf_decode_flush_many<WFlowsPolicy>(rx, "fec_rxw_flows_decode_flush_many", code, flows, nsel, 0, max_sweeps, do_ml,
                                               RxResults{out, sweeps, residual, status, erased_out, residual_src}, blocks, closes);
}

int ldpc_amd_fec_rxw_flows_info(ldpc_amd_ctx *ctx, int64_t info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_flows_info: info must not be null");
    memcpy(info, ctx->rxwf_info, sizeof(ctx->rxwf_info));
    return LDPC_AMD_OK;
}

}  // extern "C"
