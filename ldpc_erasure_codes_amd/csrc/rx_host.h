// rx_host.h -- the host code the device receivers share: wire_dev.hip (ldpc_amd_fec_rx_dev, ldpc_amd_fec_rx_flows), rx_window_dev.hip
// (ldpc_amd_fec_rxw_dev) and rx_window_flows_dev.hip (ldpc_amd_fec_rxw_flows).  No kernel and no device function lives here: each
// receiver keeps its own kernels, its plan, its commit and its info words, and hands the DECODE TAIL of a call to the driver below.
// The driver keeps two rules for all of them:
//   1. every workspace of a call is reserved (rx_decode_reserve) before anything moves, so a refusal leaves the receiver where it was;
//   2. whatever rewrites the staging planes -- the staging update (e), a flush's plane reset -- is launched by the caller BEHIND
//      rx_decode_slots: the fused decode reads the planes, the composed gather reads them chunk by chunk.
// The call skeleton of the two multi-flow receivers, in front of and around that tail, is rx_flows_host.h.
// Everything here has internal linkage: each unit that includes the header gets its own copy.
// A windowed receiver defines LDPC_AMD_RX_HOST_WINDOWED before the include and gets the window's host mirror too (the scan's
// result record, rx_window_scan_dev.h, names its words like wire_dev.hip's own record, so that unit cannot see both).
#ifndef LDPC_ERASURE_AMD_RX_HOST_H
#define LDPC_ERASURE_AMD_RX_HOST_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "internal.h"
#ifdef LDPC_AMD_RX_HOST_WINDOWED
#include "rx_window_scan_dev.h"   // the result record's words: R_BASE .. R_CNT
#endif

namespace ldpc_amd {
namespace {

constexpr size_t kRxScratchMax = (size_t)256 << 20;   // composed form: received symbols of one chunk of closed blocks

// the result arrays of a decode call, [T] slots each; all but `out` may be null
struct RxResults {
    uint8_t *out;
    int32_t *sweeps, *residual, *status;
    uint8_t *erased_out;
    int32_t *residual_src;
};

// the result arrays of slots first .. first + count - 1
inline void rx_result_slots(DecodeArgs &d, const RxResults &o, const uint8_t *er, int n, size_t frame, int first, int count)
{
    d.nframes = count;
    d.erased = er + (size_t)first * n;
    d.out = o.out + (size_t)first * frame;
    d.sweeps = o.sweeps ? o.sweeps + first : nullptr;
    d.residual = o.residual ? o.residual + first : nullptr;
    d.status = o.status ? o.status + first : nullptr;
    d.erased_out = o.erased_out ? o.erased_out + (size_t)first * n : nullptr;
    d.residual_src = o.residual_src ? o.residual_src + first : nullptr;
}

// the pinned copy of a plan's result records, grown to res_bytes; Rx: any receiver object with res_host, res_host_cap
template <class Rx>
int rx_readback_grow(ldpc_amd_ctx *ctx, Rx *rx, size_t res_bytes)
{
    if (rx->res_host_cap >= res_bytes) return LDPC_AMD_OK;
    if (rx->res_host) (void)hipHostFree(rx->res_host);   // no copy into it is pending: every plan ends with a synchronisation
    rx->res_host = nullptr;
    rx->res_host_cap = 0;
    LDPC_HIP_TRY(ctx, hipHostMalloc((void **)&rx->res_host, res_bytes, hipHostMallocDefault));
    rx->res_host_cap = res_bytes;
    return LDPC_AMD_OK;
}

// the decode calls' arguments, checked before anything is planned; Rx: any receiver object with n, k, S
template <class Rx>
int rx_decode_check(ldpc_amd_ctx *ctx, const Rx *rx, const char *who, int code, int max_sweeps, const RxResults &o)
{
    if (code < 0 || code >= (int)ctx->codes.size()) return set_error(ctx, LDPC_AMD_ENOCODE, "unknown code handle %d", code);
    const DevCode &cd = ctx->codes[code]->dev;
    if (cd.n != rx->n || cd.k != rx->k)
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: the code is (%d,%d), the receiver was created for (%d,%d)", who, cd.n, cd.k, rx->n, rx->k);
    // the decoder's own refusals (launch_decode), before anything is planned
    if (!symbol_len_ok(ctx, rx->S)) return refuse_symbol_len(ctx, rx->S, "S must be 1 or a multiple of 16 (got %d)");
    if (max_sweeps < 1) return set_error(ctx, LDPC_AMD_EINVAL, "max_sweeps must be >= 1");
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const void *opt[] = {o.sweeps, o.residual, o.status, o.erased_out, o.residual_src};
    bool ok = o.out && is_device_ptr(ctx, o.out);
    for (const void *p : opt) ok = ok && (!p || is_device_ptr(ctx, p));
    if (!ok) return set_error(ctx, LDPC_AMD_EINVAL, "%s: out and the result arrays must be device pointers of device %d", who, ctx->device);
    return LDPC_AMD_OK;
}

// ---- the decode driver ------------------------------------------------------------------------------------------------------------
// A decode call hands T closed slots of n rows to the decoder.  FUSED: a row-source kernel of the caller's (`sources`) writes one
// word and one flag per row and ONE launch_decode follows the words into the packets and the staging planes (PacketRows).  COMPOSED:
// a gather of the caller's copies a chunk of slots into the context's scratch, the decoder runs on it, next chunk; the chunks follow
// one another on the context's stream, so the scratch is free again when the next gather starts.
// Two steps, because a caller reserves before its winners' table or its plane numbers go out, and drives behind them.

// slots per chunk of the composed form; `bound`: what the entry point knows of T when it sizes (max_blocks before the plan, else T)
inline int64_t rx_chunk(int64_t bound, size_t frame) { return std::max<int64_t>(1, std::min<int64_t>(bound, (int64_t)(kRxScratchMax / frame))); }

// scratch_bytes: the received-symbol scratch of the composed form, 0 in the fused form
inline int rx_decode_reserve(ldpc_amd_ctx *ctx, int T, int n, size_t frame, bool fused, int64_t chunk, size_t *scratch_bytes)
{
    *scratch_bytes = 0;
    if (T <= 0) return LDPC_AMD_OK;
    int rc;
    if ((rc = scratch_reserve(ctx, ctx->rx_er, (size_t)T * n))) return rc;
    if (fused) return scratch_reserve(ctx, ctx->rx_src, sizeof(uint32_t) * (size_t)T * n);
    return scratch_reserve(ctx, ctx->rx_sym, *scratch_bytes = (size_t)std::min<int64_t>(chunk, T) * frame);
}

inline DecodeArgs rx_decode_args(const DevCode &cd, int n, int S, int max_sweeps, int do_ml)
{
    DecodeArgs d{};
    d.code = cd; d.S = S; d.in_rows = n; d.max_sweeps = max_sweeps; d.do_ml = do_ml ? 1 : 0;
    return d;
}

// sources(src, er): the caller's row-source launch for all T slots.  gather(first, count, sym, er): its gather of slots first ..
// first + count - 1 into sym, their flags into er.  pin: the packet and staging bases of the fused form (src is filled in here).
// launches: the launch_decode calls made.
template <class Sources, class Gather>
int rx_decode_slots(ldpc_amd_ctx *ctx, DecodeArgs &d, const RxResults &o, int T, int64_t chunk, bool fused, const PacketRows &pin,
                    Sources sources, Gather gather, int *launches)
{
    *launches = 0;
    if (T <= 0) return LDPC_AMD_OK;
    const int n = d.in_rows;
    const size_t frame = (size_t)n * d.S;
    uint8_t *er = (uint8_t *)ctx->rx_er.p;
    int rc;
    if (fused) {
        uint32_t *src = (uint32_t *)ctx->rx_src.p;
        if ((rc = sources(src, er))) return rc;
        rx_result_slots(d, o, er, n, frame, 0, T);
        d.sym = nullptr;
        d.pin = pin;
        d.pin.src = src;
        if ((rc = launch_decode(ctx, d))) return rc;
        *launches = 1;
        return LDPC_AMD_OK;
    }
    uint8_t *sym = (uint8_t *)ctx->rx_sym.p;
    for (int first = 0; first < T; first += (int)chunk) {
        const int count = (int)std::min<int64_t>(chunk, T - first);
        if ((rc = gather(first, count, sym, er + (size_t)first * n))) return rc;
        rx_result_slots(d, o, er, n, frame, first, count);
        d.sym = sym;
        if ((rc = launch_decode(ctx, d))) return rc;
        ++*launches;
    }
    return LDPC_AMD_OK;
}

// ---- the batch flushes' plane numbers -------------------------------------------------------------------------------------------------
// One int32 plane number per handed-out slot, on the device, and their pinned staging: two slots used in turn, each with the event of
// its last copy, so that a slot is never rewritten under a copy in flight.  Allocated by the first upload.
struct RxPlaneUpload {
    int32_t *dev = nullptr;
    int32_t *host[2] = {nullptr, nullptr};
    hipEvent_t event[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    unsigned calls = 0;
};

// planes[0 .. T-1] to u.dev through the pinned slot of this call; cap: the most plane numbers a call of the object uploads
inline int rx_upload_planes(ldpc_amd_ctx *ctx, const char *who, RxPlaneUpload &u, size_t cap, const int32_t *planes, int T)
{
    if (!u.dev) {
        hipError_t e = hipMalloc((void **)&u.dev, sizeof(int32_t) * cap);
        for (int s = 0; s < 2 && e == hipSuccess; s++) {
            if (!u.host[s]) e = hipHostMalloc((void **)&u.host[s], sizeof(int32_t) * cap, hipHostMallocDefault);
            if (e == hipSuccess && !u.event[s]) e = hipEventCreateWithFlags(&u.event[s], hipEventDisableTiming);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (u.dev) (void)hipFree(u.dev);
            u.dev = nullptr;   // (what the slots got is kept: the next call asks for the rest)
            return set_error(ctx, LDPC_AMD_ENOMEM, "%s: no memory for the slot descriptors: %s", who, hipGetErrorString(e));
        }
    }
    const int slot = (int)(u.calls & 1u);
    if (u.pending[slot]) {   // the copy that last read this slot (two calls ago) must be through
        LDPC_HIP_TRY(ctx, hipEventSynchronize(u.event[slot]));
        u.pending[slot] = false;
    }
    memcpy(u.host[slot], planes, sizeof(int32_t) * (size_t)T);
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(u.dev, u.host[slot], sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, ctx->stream));
    LDPC_HIP_TRY(ctx, hipEventRecord(u.event[slot], ctx->stream));
    u.pending[slot] = true;
    u.calls++;
    return LDPC_AMD_OK;
}

inline void rx_upload_free(RxPlaneUpload &u)
{
    if (u.dev) (void)hipFree(u.dev);
    for (int s = 0; s < 2; s++) {
        if (u.host[s]) (void)hipHostFree(u.host[s]);
        if (u.event[s]) (void)hipEventDestroy(u.event[s]);
    }
}

#ifdef LDPC_AMD_RX_HOST_WINDOWED
// ---- the windowed receivers' host mirror ----------------------------------------------------------------------------------------------
// One flow's state as the host keeps it (csrc/rx_window.cpp): a view onto the single object's members or onto flow f's slices.
struct RxwMirror {
    int *base, *head, *ahead;   // head: the staging plane (of the flow's W) of slot 0
    int *cnt;                   // [W]
    int64_t *totals;            // [5]
    int W;
};

inline int64_t word64(const int32_t *h, int lo) { return (int64_t)(((uint64_t)(uint32_t)h[lo + 1] << 32) | (uint32_t)h[lo]); }

// the mirror after a call that closed `closes` blocks, from the scan's result record h
inline void rxw_mirror_commit(const RxwMirror &m, const int32_t *h, int closes)
{
    *m.base = h[R_BASE]; *m.ahead = h[R_AHEAD];
    for (int j = 0; j < m.W; j++) m.cnt[j] = h[R_CNT + j];
    *m.head = (*m.head + closes) % m.W;
    m.totals[LDPC_AMD_RXW_BAD_SYMBOL] += word64(h, R_BAD_LO);
    m.totals[LDPC_AMD_RXW_LATE] += word64(h, R_LATE_LO);
    m.totals[LDPC_AMD_RXW_AHEAD] += word64(h, R_AHEADTOT_LO);
    m.totals[LDPC_AMD_RXW_RESYNCS] += h[R_RESYNCS];
    m.totals[LDPC_AMD_RXW_CLOSED] += closes;
}

// The blocks a flush hands out: every open slot up to the last non-empty one.
inline int rxw_mirror_flush_count(const int *cnt, int W)
{
    int count = 0;
    for (int d = 0; d < W; d++)
        if (cnt[d] > 0) count = d + 1;
    return count;
}

// the mirror after a flush of `count` > 0 blocks, each a close; blocks (may be null): their wire numbers
inline void rxw_mirror_flush(const RxwMirror &m, int count, int *blocks)
{
    for (int j = 0; j < count; j++)
        if (blocks) blocks[j] = (*m.base + j) & 0xff;
    for (int d = 0; d < m.W; d++) m.cnt[d] = d + count < m.W ? m.cnt[d + count] : 0;
    *m.head = (*m.head + count) % m.W;
    *m.base = (*m.base + count) & 0xff;
    *m.ahead = 0;
    m.totals[LDPC_AMD_RXW_CLOSED] += count;
}

// the create calls' window arguments; rows: the staging rows of the object, rows_text: how the caller's arguments make them up
inline int rxw_check_create(ldpc_amd_ctx *ctx, const char *who, int window, int ahead_limit, int64_t rows, const char *rows_text)
{
    if (window < LDPC_AMD_RXW_MIN_WINDOW || window > LDPC_AMD_RXW_MAX_WINDOW || ahead_limit < 0 || ahead_limit > (1 << 30))
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: need 2 <= window <= 32 and 0 <= ahead_limit <= 2^30 (window=%d ahead_limit=%d)", who, window,
                         ahead_limit);
    if (rows >= (int64_t)0x7ffffffe)
        return set_error(ctx, LDPC_AMD_EINVAL, "%s: %s = %lld staging rows, a staged-row word names fewer than 2^31 - 2", who, rows_text,
                         (long long)rows);
    return LDPC_AMD_OK;
}
#endif  // LDPC_AMD_RX_HOST_WINDOWED

}  // namespace
}  // namespace ldpc_amd

#endif  // LDPC_ERASURE_AMD_RX_HOST_H
