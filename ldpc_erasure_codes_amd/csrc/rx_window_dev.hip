// rx_window_dev.hip -- the windowed FEC receiver on the device (include/ldpc_erasure_amd_rx_window.h): csrc/rx_window.cpp's object for
// packets that are already in GPU memory, byte for byte.  The five steps of wire_dev.hip's two-buffer receiver, with W blocks open:
//   (a) rxw_headers   every packet's header -> one dense u32, block << 16 | symbol                                        (parallel)
//   (b) rxw_scan      one wavefront replays ldpc_amd_fec_rxw_push over the dense headers, 64 packets per step: per packet the
//                     SERIAL of the block it went to (or -1), per close the wire block number, at the end the state and the totals;
//                     rxw_scan_grouped for an object of depth > 1 (include/ldpc_erasure_amd_interleave.h), the only step that differs;
//                     rxw_scan_ruled / rxw_scan_grouped_ruled for an object whose close rule is not the default rule
//                     (include/ldpc_erasure_amd_rx_rule.h): the only step that looks at the rule
//   (c) rxw_winners   atomicMax of the packet index into a [(closes + W)][n] table: the last copy of a symbol wins          (parallel)
//   (d) rxw_move<1>   closed blocks -> sym_batch / erased_batch; or rxw_sources: WHERE the decoder finds each row           (parallel)
//   (e) rxw_move<0>   the W blocks still open -> the W staging planes, in a launch behind (d)                              (parallel)
// Serials: the blocks open when the call starts are serials 0 .. W-1 (slot d = serial d); the t-th close of the call (0-based)
// hands out serial t -- blocks close in the order they were opened -- and opens serial t + W.  So closed slot t of the call is serial
// t, and the blocks open at the end are serials closes .. closes + W - 1.  Serial s lives in ring plane (head + s) % W, head = the
// plane of slot 0 when the call starts.  Serials below W were carried in: their planes hold what earlier calls received; every other
// serial starts zero and erased.  The plane a new serial s >= W takes over is the plane of serial s - W, a block (d) may still read,
// hence (e) behind (d).  A re-anchor happens only when every open block is empty: it consumes no serial and moves no data; it changes
// `base`, and the packet that tripped it goes to the serial in slot 0.
// The host code around the kernels that every device receiver needs -- the argument check and the decode tail of the decode calls, the
// host mirror of the window -- is csrc/rx_host.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>

#include "../../include/ldpc_erasure_amd_rx_window.h"
#include "../../include/ldpc_erasure_amd_rs_wire.h"
#define LDPC_AMD_RX_HOST_WINDOWED
#include "rx_host.h"   // and with it rx_window_scan_dev.h, (b) the plan scan: RxwRule, RxwState, the result record, rxw_scan_body

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
__global__ __launch_bounds__(kThreads) void rxw_headers(const uint8_t *__restrict__ packets, int64_t np, int plen, uint32_t *__restrict__ dense)
{
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < np; p += (int64_t)gridDim.x * kThreads) {
        const uint8_t *h = packets + p * plen;
        uint32_t w;
        if (ALIGNED4) w = *reinterpret_cast<const uint32_t *>(h) & 0x00ffffffu;
        else w = (uint32_t)h[0] | (uint32_t)h[1] << 8 | (uint32_t)h[2] << 16;
        dense[p] = w;
    }
}

// ---- (b) the plan scan: rx_window_scan_dev.h ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rxw_scan(const uint32_t *__restrict__ dense, int64_t np, RxwRule r, int max_blocks, RxwState st,
                                              int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    __shared__ int cnt[kMaxW];
    __shared__ uint32_t hbuf[kScanChunk * 64];
    rxw_scan_body<false>(dense, np, r, 1, max_blocks, st, cnt, hbuf, dest, res);
}

// the depth-D rule (include/ldpc_erasure_amd_interleave.h), D > 1: the objects created with a depth launch this one
__global__ __launch_bounds__(64) void rxw_scan_grouped(const uint32_t *__restrict__ dense, int64_t np, RxwRule r, int D, int max_blocks,
                                                      RxwState st, int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    __shared__ int cnt[kMaxW];
    __shared__ uint32_t hbuf[kScanChunk * 64];
    rxw_scan_body<true>(dense, np, r, D, max_blocks, st, cnt, hbuf, dest, res);
}

// ---- (c) last writer wins ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void rxw_winners(const uint32_t *__restrict__ dense, const int32_t *__restrict__ dest, int64_t consumed,
                                                       int n, int32_t *__restrict__ win)
{
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < consumed; p += (int64_t)gridDim.x * kThreads) {
        const int s = dest[p];
        if (s >= 0) atomicMax(&win[(int64_t)s * n + (dense[p] & 0xffffu)], (int32_t)p);   // dest >= 0 only for symbol < n
    }
}

// ---- (d) gather into the closed slots, (e) staging planes ----------------------------------------------------------------------------
struct MoveArgs {
    const uint8_t *packets;
    int64_t plen;
    const int32_t *win;   // [(closes + W)][n]
    uint8_t *stage_sym;   // [W][n][S]
    uint8_t *stage_er;    // [W][n]
    uint8_t *sym_out;     // gather: [count][n][S], the closed slots first .. first + count - 1
    uint8_t *er_out;      // gather: [count][n]
    int n, S, W, head, closes;
    int first, count;
};

// Row r of the gather (slot = serial first + r / n, symbol i): the last packet that went there, else -- a block carried in from an
// earlier call -- its staging row, else zero and erased.  Row r of the staging update (serial closes + r / n): the last packet, else
// for a block opened in this call zero and erased; a carried block keeps its staging row.
template <bool GATHER, bool V16>
__global__ __launch_bounds__(kThreads) void rxw_move(MoveArgs a)
{
    const int q = V16 ? a.S / 16 : a.S;   // 16-byte pieces or bytes of a row
    const int64_t rows = (int64_t)(GATHER ? a.count : a.W) * a.n;
    const int64_t total = rows * q;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int64_t r = t / q;
        const int c = (int)(t - r * q);
        const int s = (int)(r / a.n) + (GATHER ? a.first : a.closes);   // serial of the block
        const int i = (int)(r - (int64_t)(r / a.n) * a.n);
        const int w = a.win[(int64_t)s * a.n + i];
        const int b = (a.head + s) % a.W;
        const bool carried = s < a.W;
        const int64_t erow = (int64_t)b * a.n + i;   // the block's staging row
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

// (d') the fused form: the gather's rule for row r as a word the packets-in decoder follows (internal.h, PacketRows) -- the W planes
// are one `stage` base, row i of plane b is staging row b * n + i -- and the erasure flag the gather would have written.
__global__ __launch_bounds__(kThreads) void rxw_sources(const int32_t *__restrict__ win, const uint8_t *__restrict__ stage_er, int n, int W,
                                                       int head, int closes, uint32_t *__restrict__ src, uint8_t *__restrict__ er)
{
    const int64_t total = (int64_t)closes * n;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < total; r += (int64_t)gridDim.x * kThreads) {
        const int s = (int)(r / n);
        const int i = (int)(r - (int64_t)s * n);
        const int w = win[r];
        const int row = ((head + s) % W) * n + i;   // W * n < 2^31 - 2 (create)
        uint32_t word = kRowErased;
        if (w >= 0) word = (uint32_t)w;
        else if (s < W && stage_er[row] == 0) word = kRowStaged | (uint32_t)row;
        src[r] = word;
        er[r] = word == kRowErased ? 1 : 0;
    }
}

// ---- flush: slots first .. first + count - 1 of the window lie complete in their planes.  Grid (x, count): plane -> dense slot, and the
// plane back to symbols 0 / flags 1, one work item per piece of PW bytes (16 or 1; PW divides S, so a plane has at least n pieces:
// piece u < n also moves flag u).  Each piece and flag is read and rewritten by one work item only.
template <int PW>
__global__ __launch_bounds__(kThreads) void rxw_flush_move(uint8_t *__restrict__ stage_sym, uint8_t *__restrict__ stage_er, int n, int S, int W,
                                                          int head, int first, uint8_t *__restrict__ sym_out, uint8_t *__restrict__ er_out)
{
    const int64_t upp = (int64_t)n * S / PW;   // pieces of a plane
    const int64_t s = blockIdx.y, plane = (head + first + s) % W;
    uint8_t *from = stage_sym + plane * upp * PW;
    uint8_t *to = sym_out + s * upp * PW;
    for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < upp; u += (int64_t)gridDim.x * kThreads) {
        if (PW == 16) {
            reinterpret_cast<uint4 *>(to)[u] = reinterpret_cast<const uint4 *>(from)[u];
            reinterpret_cast<uint4 *>(from)[u] = make_uint4(0, 0, 0, 0);
        } else {
            to[u] = from[u];
            from[u] = 0;
        }
        if (u < n) {
            er_out[s * n + u] = stage_er[plane * n + u];
            stage_er[plane * n + u] = 1;
        }
    }
}

// ---- (b) for an object whose close rule is not the default rule (include/ldpc_erasure_amd_rx_rule.h): the same scan with step 3's
// four thresholds read from its argument, plain and grouped.  They stand behind the other kernels of the unit so that theirs keep
// their places in the code object.
__global__ __launch_bounds__(64) void rxw_scan_ruled(const uint32_t *__restrict__ dense, int64_t np, RxwRuleV r, int max_blocks, RxwState st,
                                                    int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    __shared__ int cnt[kMaxW];
    __shared__ uint32_t hbuf[kScanChunk * 64];
    rxw_scan_body<false>(dense, np, r, 1, max_blocks, st, cnt, hbuf, dest, res);
}

__global__ __launch_bounds__(64) void rxw_scan_grouped_ruled(const uint32_t *__restrict__ dense, int64_t np, RxwRuleV r, int D, int max_blocks,
                                                            RxwState st, int32_t *__restrict__ dest, int32_t *__restrict__ res)
{
    __shared__ int cnt[kMaxW];
    __shared__ uint32_t hbuf[kScanChunk * 64];
    rxw_scan_body<true>(dense, np, r, D, max_blocks, st, cnt, hbuf, dest, res);
}

}  // namespace

struct ldpc_amd_fec_rxw_dev {
    ldpc_amd_ctx *ctx = nullptr;
    int n = 0, k = 0, S = 0, W = 0, A = 0, kd = 0, km = 0;
    int D = 1;   // interleaving depth (include/ldpc_erasure_amd_interleave.h); only the plan scan looks at it
    ldpc_amd_fec_rx_rule rule{};   // the close rule (include/ldpc_erasure_amd_rx_rule.h); only the plan scan looks at it
    bool ruled = false;            // the rule is not the default rule: the ruled scan kernels (else kd, km and the kernels there always were)
    // host mirror of the receiver's state (csrc/rx_window.cpp); head: staging plane of slot 0
    int base = -1, head = 0, ahead = 0;
    int cnt[kMaxW] = {0};
    int64_t totals[5] = {0, 0, 0, 0, 0};
    uint8_t *stage_sym = nullptr;   // [W][n][S]
    uint8_t *stage_er = nullptr;    // [W][n]
    Scratch dense, dest, win, res;  // per-call scratch, grown on demand
    int32_t *res_host = nullptr;    // pinned copy of res
    size_t res_host_cap = 0;
};

namespace {

// One call's PLAN: (a) + (b) and the read-back.  Nothing of the receiver's state changes before rxw_commit.
struct RxwPlan {
    int closes = 0;
    int64_t used = 0;
    const int32_t *h = nullptr;   // the scan's result record (pinned)
};

inline RxwMirror rxw_mirror(ldpc_amd_fec_rxw_dev *rx) { return RxwMirror{&rx->base, &rx->head, &rx->ahead, rx->cnt, rx->totals, rx->W}; }

int rxw_plan(ldpc_amd_fec_rxw_dev *rx, const char *who, const uint8_t *packets, int64_t npackets, int max_blocks, RxwPlan &pl)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n;
    const int64_t plen = (int64_t)rx->S + kHdr;
    const size_t res_bytes = sizeof(int32_t) * ((size_t)R_WORDS + (size_t)max_blocks);
    int rc;
    if ((rc = scratch_reserve(ctx, rx->dense, sizeof(uint32_t) * (size_t)npackets)) ||
        (rc = scratch_reserve(ctx, rx->dest, sizeof(int32_t) * (size_t)npackets)) ||
        (rc = scratch_reserve(ctx, rx->win, sizeof(int32_t) * ((size_t)max_blocks + (size_t)rx->W) * (size_t)n)) ||
        (rc = scratch_reserve(ctx, rx->res, res_bytes)))
        return rc;
    if ((rc = rx_readback_grow(ctx, rx, res_bytes))) return rc;
    uint32_t *dense = (uint32_t *)rx->dense.p;
    int32_t *dest = (int32_t *)rx->dest.p, *res = (int32_t *)rx->res.p;
    if (plen % 4 == 0 && ((uintptr_t)packets & 3) == 0)
        hipLaunchKernelGGL(rxw_headers<true>, dim3(grid_for(npackets)), dim3(kThreads), 0, ctx->stream, packets, npackets, (int)plen, dense);
    else
        hipLaunchKernelGGL(rxw_headers<false>, dim3(grid_for(npackets)), dim3(kThreads), 0, ctx->stream, packets, npackets, (int)plen, dense);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    RxwRule r{n, rx->kd, rx->km, rx->W, rx->A};
    RxwState st{};
    st.base = rx->base; st.ahead = rx->ahead;
    for (int j = 0; j < rx->W; j++) st.cnt[j] = rx->cnt[j];
    if (rx->ruled) {
        const RxwRuleV rv{n, rx->rule.c_hi, rx->rule.later_hi, rx->rule.c_lo, rx->rule.later_lo, rx->W, rx->A};
        if (rx->D > 1)
            hipLaunchKernelGGL(rxw_scan_grouped_ruled, dim3(1), dim3(64), 0, ctx->stream, dense, npackets, rv, rx->D, max_blocks, st, dest, res);
        else
            hipLaunchKernelGGL(rxw_scan_ruled, dim3(1), dim3(64), 0, ctx->stream, dense, npackets, rv, max_blocks, st, dest, res);
    } else if (rx->D > 1)
        hipLaunchKernelGGL(rxw_scan_grouped, dim3(1), dim3(64), 0, ctx->stream, dense, npackets, r, rx->D, max_blocks, st, dest, res);
    else
        hipLaunchKernelGGL(rxw_scan, dim3(1), dim3(64), 0, ctx->stream, dense, npackets, r, max_blocks, st, dest, res);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(rx->res_host, res, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    LDPC_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = check_device_error(ctx))) return rc;
    const int32_t *h = rx->res_host;
    if (h[R_ERR])
        return set_error(ctx, LDPC_AMD_EHIP, "%s: the plan scan hit its iteration cap (internal error); the receiver's state is unchanged", who);
    pl.h = h;
    pl.closes = h[R_CLOSES];
    pl.used = word64(h, R_CONSUMED_LO);
    return LDPC_AMD_OK;
}

// (c): the winners' table of the call, [(closes + W)][n]
int rxw_winners_launch(ldpc_amd_fec_rxw_dev *rx, const RxwPlan &pl)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    int32_t *win = (int32_t *)rx->win.p;
    LDPC_HIP_TRY(ctx, hipMemsetAsync(win, 0xff, sizeof(int32_t) * ((size_t)pl.closes + (size_t)rx->W) * (size_t)rx->n, ctx->stream));   // -1: no packet
    hipLaunchKernelGGL(rxw_winners, dim3(grid_for(pl.used)), dim3(kThreads), 0, ctx->stream, (const uint32_t *)rx->dense.p,
                       (const int32_t *)rx->dest.p, pl.used, rx->n, win);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

// (d) for the closed slots first .. first + count - 1 (gather) or (e) for the W open blocks
template <bool GATHER>
int rxw_move_launch(ldpc_amd_fec_rxw_dev *rx, const RxwPlan &pl, const uint8_t *packets, int first, int count, uint8_t *sym, uint8_t *er)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n, S = rx->S;
    if (GATHER && count <= 0) return LDPC_AMD_OK;
    MoveArgs a{};
    a.packets = packets; a.plen = (int64_t)S + kHdr; a.win = (const int32_t *)rx->win.p; a.stage_sym = rx->stage_sym; a.stage_er = rx->stage_er;
    a.sym_out = sym; a.er_out = er; a.n = n; a.S = S; a.W = rx->W; a.head = rx->head; a.closes = pl.closes; a.first = first; a.count = count;
    const bool v16 = S % 16 == 0 && ((uintptr_t)packets & 7) == 0 && ((uintptr_t)sym & 15) == 0;
    const int64_t items = (int64_t)(GATHER ? count : rx->W) * n * (v16 ? S / 16 : S);
    if (v16) hipLaunchKernelGGL((rxw_move<GATHER, true>), dim3(grid_for(items)), dim3(kThreads), 0, ctx->stream, a);
    else hipLaunchKernelGGL((rxw_move<GATHER, false>), dim3(grid_for(items)), dim3(kThreads), 0, ctx->stream, a);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

void rxw_commit(ldpc_amd_fec_rxw_dev *rx, const RxwPlan &pl, int *blocks, int64_t *consumed)
{
    rxw_mirror_commit(rxw_mirror(rx), pl.h, pl.closes);
    if (blocks) memcpy(blocks, pl.h + R_WORDS, sizeof(int) * (size_t)pl.closes);
    if (consumed) *consumed = pl.used;
}

// slots first .. first + count - 1 of the window -> sym / er, their planes reset: one launch
int rxw_flush_launch(ldpc_amd_fec_rxw_dev *rx, int first, int count, uint8_t *sym, uint8_t *er)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    const int n = rx->n, S = rx->S;
    const bool v16 = S % 16 == 0 && ((uintptr_t)sym & 15) == 0;
    const int64_t pieces = (int64_t)n * (v16 ? S / 16 : S);
    const dim3 grid((unsigned)std::min<int64_t>((pieces + kThreads - 1) / kThreads, 65535), (unsigned)count);
    if (v16) hipLaunchKernelGGL(rxw_flush_move<16>, grid, dim3(kThreads), 0, ctx->stream, rx->stage_sym, rx->stage_er, n, S, rx->W, rx->head, first, sym, er);
    else hipLaunchKernelGGL(rxw_flush_move<1>, grid, dim3(kThreads), 0, ctx->stream, rx->stage_sym, rx->stage_er, n, S, rx->W, rx->head, first, sym, er);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

}  // namespace

extern "C" {

int ldpc_amd_fec_rxw_dev_create(ldpc_amd_ctx *ctx, int n, int k, int S, int window, int ahead_limit, ldpc_amd_fec_rxw_dev **out)
{
    return ldpc_amd_fec_rxw_dev_create_rule(ctx, n, k, S, window, ahead_limit, 1, nullptr, out);
}

int ldpc_amd_fec_rxw_dev_depth(const ldpc_amd_fec_rxw_dev *rx) { return rx ? rx->D : -1; }

int ldpc_amd_fec_rxw_dev_get_rule(const ldpc_amd_fec_rxw_dev *rx, ldpc_amd_fec_rx_rule *rule)
{
    if (!rx || !rule) return LDPC_AMD_EINVAL;
    *rule = rx->rule;
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_rxw_dev_create_depth(ldpc_amd_ctx *ctx, int n, int k, int S, int window, int ahead_limit, int depth, ldpc_amd_fec_rxw_dev **out)
{
    return ldpc_amd_fec_rxw_dev_create_rule(ctx, n, k, S, window, ahead_limit, depth, nullptr, out);
}

int ldpc_amd_fec_rxw_dev_create_rule(ldpc_amd_ctx *ctx, int n, int k, int S, int window, int ahead_limit, int depth,
                                     const ldpc_amd_fec_rx_rule *rule, ldpc_amd_fec_rxw_dev **out)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!out || n <= 0 || n > 65536 || k <= 0 || k >= n || S <= 0)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_create: need n <= 65536, 0 < k < n, S >= 1 (n=%d k=%d S=%d)", n, k, S);
    int rc;
    if ((rc = rxw_check_create(ctx, "fec_rxw_dev_create", window, ahead_limit, (int64_t)window * n, "window * n"))) return rc;
    if (!LDPC_AMD_FEC_ILV_DEPTH_OK(depth) || (depth > 1 && 2 * depth > window))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_create: depth must be 1, 2, 4, 8 or 16, and a depth > 1 needs 2 * depth <= window (depth=%d window=%d)",
                         depth, window);
    ldpc_amd_fec_rx_rule rl{};
    bool ruled = false;
    if (rxw_rule_resolve(n, k, rule, &rl, &ruled))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_create: invalid close rule (%d, %d, %d, %d): need 0 <= c <= n = %d, 0 <= later <= 2^30, and later >= 1 where c == 0",
                         rl.c_hi, rl.later_hi, rl.c_lo, rl.later_lo, n);
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ldpc_amd_fec_rxw_dev *rx = new (std::nothrow) ldpc_amd_fec_rxw_dev();
    if (!rx) return set_error(ctx, LDPC_AMD_ENOMEM, "fec_rxw_dev_create: out of host memory");
    rx->ctx = ctx;
    rx->n = n; rx->k = k; rx->S = S; rx->W = window; rx->A = ahead_limit; rx->D = depth;
    rx->rule = rl; rx->ruled = ruled;
    rx->kd = k + (int)lround((n - k) * 0.8);
    rx->km = k + (int)lround((n - k) * 0.2);
    const size_t planes = (size_t)window * n * S, flags = (size_t)window * n;
    hipError_t e = hipMalloc((void **)&rx->stage_sym, planes);
    if (e == hipSuccess) e = hipMalloc((void **)&rx->stage_er, flags);
    if (e == hipSuccess) e = hipMemsetAsync(rx->stage_sym, 0, planes, ctx->stream);   // payload zero, every symbol erased
    if (e == hipSuccess) e = hipMemsetAsync(rx->stage_er, 1, flags, ctx->stream);
    if (e != hipSuccess) {
        ldpc_amd_fec_rxw_dev_destroy(rx);
        return set_error(ctx, e == hipErrorOutOfMemory ? LDPC_AMD_ENOMEM : LDPC_AMD_EHIP, "fec_rxw_dev_create: %s", hipGetErrorString(e));
    }
    *out = rx;
    return LDPC_AMD_OK;
}

void ldpc_amd_fec_rxw_dev_destroy(ldpc_amd_fec_rxw_dev *rx)
{
    if (!rx) return;
    (void)hipSetDevice(rx->ctx->device);
    (void)hipStreamSynchronize(rx->ctx->stream);   // pending work of this receiver may still use its buffers
    Scratch *sc[] = {&rx->dense, &rx->dest, &rx->win, &rx->res};
    for (Scratch *s : sc)
        if (s->p) (void)hipFree(s->p);
    if (rx->stage_sym) (void)hipFree(rx->stage_sym);
    if (rx->stage_er) (void)hipFree(rx->stage_er);
    if (rx->res_host) (void)hipHostFree(rx->res_host);
    delete rx;
}

int ldpc_amd_fec_rxw_dev_stats(const ldpc_amd_fec_rxw_dev *rx, int64_t totals[5])
{
    if (!rx || !totals) return LDPC_AMD_EINVAL;
    memcpy(totals, rx->totals, sizeof(rx->totals));
    return LDPC_AMD_OK;
}

int64_t ldpc_amd_fec_rxw_dev_dropped(const ldpc_amd_fec_rxw_dev *rx)
{
    return rx ? rx->totals[LDPC_AMD_RXW_BAD_SYMBOL] + rx->totals[LDPC_AMD_RXW_LATE] + rx->totals[LDPC_AMD_RXW_AHEAD] : -1;
}

int ldpc_amd_fec_rxw_dev_state(const ldpc_amd_fec_rxw_dev *rx, int *base, int *cnt, int64_t *ahead)
{
    if (!rx) return LDPC_AMD_EINVAL;
    if (base) *base = rx->base;
    if (cnt) memcpy(cnt, rx->cnt, sizeof(int) * (size_t)rx->W);
    if (ahead) *ahead = rx->ahead;
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_rxw_dev_push_many(ldpc_amd_fec_rxw_dev *rx, const uint8_t *packets, int64_t npackets, uint8_t *sym_batch,
                                   uint8_t *erased_batch, int *blocks, int max_blocks, int64_t *consumed)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    if (npackets < 0 || npackets >= ((int64_t)1 << 31) || max_blocks < 1)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_push_many: need 0 <= npackets < 2^31 and max_blocks >= 1");
    if (!sym_batch || !erased_batch || (npackets > 0 && !packets))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_push_many: packets / sym_batch / erased_batch must not be null");
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((npackets > 0 && !is_device_ptr(ctx, packets)) || !is_device_ptr(ctx, sym_batch) || !is_device_ptr(ctx, erased_batch))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_push_many: packets / sym_batch / erased_batch must be device pointers of device %d",
                         ctx->device);
    if (consumed) *consumed = 0;
    if (npackets == 0) return 0;
    int rc;
    RxwPlan pl;
    if ((rc = rxw_plan(rx, "fec_rxw_dev_push_many", packets, npackets, max_blocks, pl))) return rc;
    if ((rc = rxw_winners_launch(rx, pl)) || (rc = rxw_move_launch<true>(rx, pl, packets, 0, pl.closes, sym_batch, erased_batch)) ||
        (rc = rxw_move_launch<false>(rx, pl, packets, 0, 0, sym_batch, nullptr)))
        return rc;
    rxw_commit(rx, pl, blocks, consumed);
    return pl.closes;
}

int ldpc_amd_fec_rxw_dev_flush(ldpc_amd_fec_rxw_dev *rx, uint8_t *sym_batch, uint8_t *erased_batch, int *blocks)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    const int count = rxw_mirror_flush_count(rx->cnt, rx->W);
    if (count == 0) return 0;
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!sym_batch || !erased_batch || !is_device_ptr(ctx, sym_batch) || !is_device_ptr(ctx, erased_batch))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_flush: sym_batch / erased_batch must be device pointers of device %d", ctx->device);
    int rc;
    if ((rc = rxw_flush_launch(rx, 0, count, sym_batch, erased_batch))) return rc;
    rxw_mirror_flush(rxw_mirror(rx), count, blocks);
    return count;
}

// push_many + decode_frames in one call (rx_host.h: the decode driver).  FUSED where the decoder can fetch its rows from the packets
// itself (decode_reads_packets): (d) shrinks to rxw_sources, the W planes being one `stage` base.  Else COMPOSED: (d) gathers chunk by
// chunk.  (e) is launched BEHIND the decode in both forms: it overwrites the staging planes of the carried blocks, which the fused
// decode reads.
int ldpc_amd_fec_rxw_dev_decode_many(ldpc_amd_fec_rxw_dev *rx, int code, const uint8_t *packets, int64_t npackets, int max_sweeps,
                                     int do_ml, uint8_t *out, int32_t *sweeps, int32_t *residual, int32_t *status,
                                     uint8_t *erased_out, int32_t *residual_src, int *blocks, int max_blocks, int64_t *consumed)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    if (code < 0 || code >= (int)ctx->codes.size()) return set_error(ctx, LDPC_AMD_ENOCODE, "unknown code handle %d", code);
    if (npackets < 0 || npackets >= ((int64_t)1 << 31) || max_blocks < 1)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_decode_many: need 0 <= npackets < 2^31 and max_blocks >= 1");
    if (npackets == 0) {
        if (consumed) *consumed = 0;
        return 0;
    }
    int rc;
    const RxResults o{out, sweeps, residual, status, erased_out, residual_src};
    if ((rc = rx_decode_check(ctx, rx, "fec_rxw_dev_decode_many", code, max_sweeps, o))) return rc;
    if (!packets || !is_device_ptr(ctx, packets))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_decode_many: packets must be a device pointer of device %d", ctx->device);
    const DevCode &cd = ctx->codes[code]->dev;
    const int n = rx->n, S = rx->S;
    const bool fused = ctx->knobs.rx_pkt != 0 && ((uintptr_t)packets & 7) == 0 && decode_reads_packets(ctx, cd, S);
    const size_t frame = (size_t)n * S;
    const int64_t chunk = rx_chunk(max_blocks, frame);

    RxwPlan pl;
    if ((rc = rxw_plan(rx, "fec_rxw_dev_decode_many", packets, npackets, max_blocks, pl))) return rc;
    const int closes = pl.closes;
    size_t scratch = 0;
    if ((rc = rx_decode_reserve(ctx, closes, n, frame, fused, chunk, &scratch))) return rc;
    if ((rc = rxw_winners_launch(rx, pl))) return rc;
    DecodeArgs d = rx_decode_args(cd, n, S, max_sweeps, do_ml);
    const PacketRows pin{nullptr, packets, rx->stage_sym, S + kHdr};
    auto sources = [&](uint32_t *src, uint8_t *er) -> int {
        hipLaunchKernelGGL(rxw_sources, dim3(grid_for((int64_t)closes * n)), dim3(kThreads), 0, ctx->stream, (const int32_t *)rx->win.p,
                           rx->stage_er, n, rx->W, rx->head, closes, src, er);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        return LDPC_AMD_OK;
    };
    auto gather = [&](int first, int count, uint8_t *sym, uint8_t *er) { return rxw_move_launch<true>(rx, pl, packets, first, count, sym, er); };
    int launches = 0;
    if ((rc = rx_decode_slots(ctx, d, o, closes, chunk, fused, pin, sources, gather, &launches))) return rc;
    if ((rc = rxw_move_launch<false>(rx, pl, packets, 0, 0, nullptr, nullptr))) return rc;   // (e)
    rxw_commit(rx, pl, blocks, consumed);
    ctx->rxw_info[0] = fused ? 1 : 2; ctx->rxw_info[1] = closes; ctx->rxw_info[2] = launches; ctx->rxw_info[3] = (int64_t)scratch;
    return closes;
}

// flush + decode, composed: the blocks lie complete in their planes, a chunk of them goes to the scratch (its planes reset by the same
// launch) and through the decoder
int ldpc_amd_fec_rxw_dev_decode_flush(ldpc_amd_fec_rxw_dev *rx, int code, int max_sweeps, int do_ml, uint8_t *out, int32_t *sweeps,
                                      int32_t *residual, int32_t *status, uint8_t *erased_out, int32_t *residual_src, int *blocks)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    int rc;
    const RxResults o{out, sweeps, residual, status, erased_out, residual_src};
    if ((rc = rx_decode_check(ctx, rx, "fec_rxw_dev_decode_flush", code, max_sweeps, o))) return rc;
    const int count = rxw_mirror_flush_count(rx->cnt, rx->W);
    if (count == 0) return 0;
    const int n = rx->n;
    const size_t frame = (size_t)n * rx->S;
    const int64_t chunk = rx_chunk(count, frame);
    size_t scratch = 0;
    if ((rc = rx_decode_reserve(ctx, count, n, frame, false, chunk, &scratch))) return rc;
    DecodeArgs d = rx_decode_args(ctx->codes[code]->dev, n, rx->S, max_sweeps, do_ml);
    auto sources = [](uint32_t *, uint8_t *) -> int { return LDPC_AMD_OK; };   // (never fused)
    auto gather = [&](int first, int c, uint8_t *sym, uint8_t *er) { return rxw_flush_launch(rx, first, c, sym, er); };
    int launches = 0;
    if ((rc = rx_decode_slots(ctx, d, o, count, chunk, false, PacketRows{}, sources, gather, &launches))) return rc;
    rxw_mirror_flush(rxw_mirror(rx), count, blocks);
    ctx->rxw_info[0] = 2; ctx->rxw_info[1] = count; ctx->rxw_info[2] = launches; ctx->rxw_info[3] = (int64_t)scratch;
    return count;
}

}  // extern "C"

// ---- the RS decode tail (include/ldpc_erasure_amd_rs_wire.h) -------------------------------------------------------------------------
// The checks both RS calls share.  *r: the code.
static int rxw_rs_check(ldpc_amd_fec_rxw_dev *rx, const char *who, int rs, uint8_t *msg, int32_t *received, int32_t *status, uint8_t *erased_batch,
                        const HostRs **r)
{
    ldpc_amd_ctx *ctx = rx->ctx;
    if (rs < 0 || rs >= (int)ctx->rs.size()) return set_error(ctx, LDPC_AMD_ENOCODE, "unknown RS handle %d", rs);
    *r = ctx->rs[rs];
    if ((*r)->n != rx->n || (*r)->k != rx->k)
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: the RS code is (%d,%d), the receiver was created for (%d,%d)", who, (*r)->n, (*r)->k, rx->n, rx->k);
    if (!symbol_len_ok(ctx, rx->S)) return refuse_symbol_len(ctx, rx->S, "S must be 1 or a multiple of 16 (got %d)");
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const void *opt[] = {received, status, erased_batch};
    bool ok = msg && is_device_ptr(ctx, msg);
    for (const void *p : opt) ok = ok && (!p || is_device_ptr(ctx, p));
    if (!ok) return set_error(ctx, LDPC_AMD_EINVAL, "%s: msg and the result arrays must be device pointers of device %d", who, ctx->device);
    return LDPC_AMD_OK;
}

// Everything T blocks of the call will need (rx_host.h, rule 1): the flags unless the caller takes them, the received symbols of one
// chunk, and what launch_rs_decode_frames reserves for a chunk -- the selection, the malformed-block counter, the generic kernel's rows.
static int rxw_rs_reserve(ldpc_amd_ctx *ctx, const HostRs &r, int S, int T, int64_t chunk, bool own_flags, size_t *scratch_bytes)
{
    *scratch_bytes = 0;
    if (T <= 0) return LDPC_AMD_OK;
    const size_t count = (size_t)std::min<int64_t>(chunk, T);
    int rc;
    if (own_flags && (rc = scratch_reserve(ctx, ctx->rx_er, (size_t)T * r.n))) return rc;
    if ((rc = scratch_reserve(ctx, ctx->rx_sym, *scratch_bytes = count * (size_t)r.n * S))) return rc;
    const size_t o_idx = (sizeof(int32_t) * count + 255) & ~(size_t)255;
    if ((rc = scratch_reserve(ctx, ctx->rssel, o_idx + count * r.k * sizeof(uint16_t))) || (rc = scratch_reserve(ctx, ctx->rsbad, 64))) return rc;
    if (S != 1 && (rc = scratch_reserve(ctx, ctx->rsws, std::min(count, (size_t)ctx->sm_count * 4) * (size_t)(r.n - r.k) * S))) return rc;
    return LDPC_AMD_OK;
}

// gather(first, count, sym, er) a chunk of the T handed-out blocks, RS-decode it, next chunk
template <class Gather>
static int rxw_rs_slots(ldpc_amd_ctx *ctx, const HostRs &r, int S, int T, int64_t chunk, uint8_t *er, uint8_t *msg, int32_t *received, int32_t *status,
                        Gather gather, int *launches)
{
    *launches = 0;
    uint8_t *sym = (uint8_t *)ctx->rx_sym.p;
    int rc;
    for (int first = 0; first < T; first += (int)chunk) {
        const int count = (int)std::min<int64_t>(chunk, T - first);
        if ((rc = gather(first, count, sym, er + (size_t)first * r.n))) return rc;
        if ((rc = launch_rs_decode_frames(ctx, r, S, count, sym, er + (size_t)first * r.n, msg + (size_t)first * r.k * S, received ? received + first : nullptr,
                                          status ? status + first : nullptr)))
            return rc;
        ++*launches;
    }
    return LDPC_AMD_OK;
}

extern "C" {

// push_many + rs_decode_frames in one call.  FUSED where the RS decoder on rows in place applies (rs_decode_rows_fused): (d) shrinks to
// rxw_sources, which also writes the flags, and the decoder follows the words into the packets and the W planes, one `stage` base.
// Else COMPOSED: (d) gathers the closed blocks chunk by chunk into the context's scratch, the RS decoder follows each chunk.  (e) behind
// the decode in both forms, as in decode_many.
int ldpc_amd_fec_rxw_dev_rs_decode_many(ldpc_amd_fec_rxw_dev *rx, int rs, const uint8_t *packets, int64_t npackets, uint8_t *msg,
                                        int32_t *received, int32_t *status, uint8_t *erased_batch, int *blocks, int max_blocks,
                                        int64_t *consumed)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    if (rs < 0 || rs >= (int)ctx->rs.size()) return set_error(ctx, LDPC_AMD_ENOCODE, "unknown RS handle %d", rs);
    if (npackets < 0 || npackets >= ((int64_t)1 << 31) || max_blocks < 1)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_rs_decode_many: need 0 <= npackets < 2^31 and max_blocks >= 1");
    const HostRs *r = nullptr;
    int rc;
    if ((rc = rxw_rs_check(rx, "fec_rxw_dev_rs_decode_many", rs, msg, received, status, erased_batch, &r))) return rc;
    if (consumed) *consumed = 0;
    if (npackets == 0) return 0;
    if (!packets || !is_device_ptr(ctx, packets))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_dev_rs_decode_many: packets must be a device pointer of device %d", ctx->device);
    const int n = rx->n, S = rx->S;
    const bool fused = rs_decode_rows_fused(ctx, *r, S, packets, rx->stage_sym, msg);
    const int64_t chunk = rx_chunk(max_blocks, (size_t)n * S);

    RxwPlan pl;
    if ((rc = rxw_plan(rx, "fec_rxw_dev_rs_decode_many", packets, npackets, max_blocks, pl))) return rc;
    const int closes = pl.closes;
    size_t scratch = 0;
    if (fused) {   // the flags unless the caller takes them, the source words, the decoder's tables
        size_t tables = 0;
        if (closes > 0 && ((!erased_batch && (rc = scratch_reserve(ctx, ctx->rx_er, (size_t)closes * n))) ||
                           (rc = scratch_reserve(ctx, ctx->rx_src, sizeof(uint32_t) * (size_t)closes * n)) ||
                           (rc = rs_decode_rows_reserve(ctx, *r, closes, &tables))))
            return rc;
        scratch = closes > 0 ? sizeof(uint32_t) * (size_t)closes * n + tables : 0;
    } else if ((rc = rxw_rs_reserve(ctx, *r, S, closes, chunk, erased_batch == nullptr, &scratch))) {
        return rc;
    }
    if ((rc = rxw_winners_launch(rx, pl))) return rc;
    uint8_t *er = erased_batch ? erased_batch : (uint8_t *)ctx->rx_er.p;
    int launches = 0;
    if (fused && closes > 0) {
        uint32_t *src = (uint32_t *)ctx->rx_src.p;
        hipLaunchKernelGGL(rxw_sources, dim3(grid_for((int64_t)closes * n)), dim3(kThreads), 0, ctx->stream, (const int32_t *)rx->win.p,
                           rx->stage_er, n, rx->W, rx->head, closes, src, er);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        // (every word rxw_sources writes lies inside the call's packets or the W planes: the decoder's own flags would be these)
        if ((rc = launch_rs_decode_rows(ctx, *r, S, closes, PacketRows{src, packets, rx->stage_sym, S + kHdr}, npackets, (int64_t)rx->W * n, nullptr,
                                        msg, received, status, &launches)))
            return rc == kDecodeNotFused ? set_error(ctx, LDPC_AMD_EHIP, "fec_rxw_dev_rs_decode_many: the row decoder refused a call it had accepted (internal error)") : rc;
    } else if (!fused) {
        auto gather = [&](int first, int count, uint8_t *sym, uint8_t *e) { return rxw_move_launch<true>(rx, pl, packets, first, count, sym, e); };
        if ((rc = rxw_rs_slots(ctx, *r, S, closes, chunk, er, msg, received, status, gather, &launches))) return rc;
    }
    if ((rc = rxw_move_launch<false>(rx, pl, packets, 0, 0, nullptr, nullptr))) return rc;   // (e)
    rxw_commit(rx, pl, blocks, consumed);
    ctx->rsrx_info[0] = closes; ctx->rsrx_info[1] = launches; ctx->rsrx_info[2] = (int64_t)scratch; ctx->rsrx_info[3] = fused ? 1 : 2;
    return closes;
}

// flush + RS decode, never fused: the blocks lie complete in their planes, a chunk of them goes to the scratch (its planes reset by the
// same launch) and through the RS decoder
int ldpc_amd_fec_rxw_dev_rs_decode_flush(ldpc_amd_fec_rxw_dev *rx, int rs, uint8_t *msg, int32_t *received, int32_t *status,
                                         uint8_t *erased_batch, int *blocks)
{
    if (!rx) return LDPC_AMD_EINVAL;
    ldpc_amd_ctx *ctx = rx->ctx;
    const HostRs *r = nullptr;
    int rc;
    if ((rc = rxw_rs_check(rx, "fec_rxw_dev_rs_decode_flush", rs, msg, received, status, erased_batch, &r))) return rc;
    const int count = rxw_mirror_flush_count(rx->cnt, rx->W);
    if (count == 0) return 0;
    const int S = rx->S;
    const int64_t chunk = rx_chunk(count, (size_t)rx->n * S);
    size_t scratch = 0;
    if ((rc = rxw_rs_reserve(ctx, *r, S, count, chunk, erased_batch == nullptr, &scratch))) return rc;
    uint8_t *er = erased_batch ? erased_batch : (uint8_t *)ctx->rx_er.p;
    auto gather = [&](int first, int c, uint8_t *sym, uint8_t *e) { return rxw_flush_launch(rx, first, c, sym, e); };
    int launches = 0;
    if ((rc = rxw_rs_slots(ctx, *r, S, count, chunk, er, msg, received, status, gather, &launches))) return rc;
    rxw_mirror_flush(rxw_mirror(rx), count, blocks);
    ctx->rsrx_info[0] = count; ctx->rsrx_info[1] = launches; ctx->rsrx_info[2] = (int64_t)scratch; ctx->rsrx_info[3] = 2;
    return count;
}

int ldpc_amd_fec_rs_receiver_info(ldpc_amd_ctx *ctx, int64_t info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_rs_receiver_info: info must not be null");
    memcpy(info, ctx->rsrx_info, sizeof(ctx->rsrx_info));
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_rxw_info(ldpc_amd_ctx *ctx, int64_t info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_rxw_info: info must not be null");
    memcpy(info, ctx->rxw_info, sizeof(ctx->rxw_info));
    return LDPC_AMD_OK;
}

}  // extern "C"
