// datagram_dev.hip -- datagrams of any length in front of the sender and behind the receiver (include/ldpc_erasure_amd_datagrams.h):
// pack datagrams into length-carrying source symbols, cut the delivered datagrams back out of decoded frames, and the host
// arithmetic of the bytes a wire packet needs.
//
// Reference: OpenCL/device/ldpc_erasure_encoder_VITA_in_UDP_out.cl:140-162 -- the sender takes every packet's length from the packet
// (packetLen = (din & 0xffff) + 2) and recomputes num_longs_used per packet; context packets have 28 words, data packets 367.
//
// A datagram symbol: S bytes, bytes 0..3 = L (little-endian u32), bytes 4..4+L-1 the datagram, the rest zero; L == 0 is a filler.
//
// PACK, one launch.  A row is S / 4 dwords; dword 0 is L, dword j >= 1 holds datagram bytes 4 (j - 1) .. 4 (j - 1) + 3.  The
// destination is 4-byte aligned, the datagram starts at any byte phase ph of an aligned dword: a lane loads the two aligned dwords
// its four bytes straddle and funnel-shifts them by ph bytes (v_alignbyte); only aligned dwords that contain a byte of the datagram
// are loaded, bytes at or behind L are masked to zero, so the zero fill is part of the same store.  Rows are dealt to groups of G
// lanes, G = 64 for rows of more than 32 dwords, else the power of two that covers the row (64 / G rows per wavefront): every row
// costs its S bytes of stores whatever L is, nothing waits for anything (no barrier, no LDS), so a wavefront that drew fillers or
// context packets is through with them after its stores and takes its next rows while another still streams a long one.
//
// UNPACK, three launches, no workgroup ever waits for another:
//   (a) dgram_unpack_lens   per row: state and length (0 unless delivered); per tile of 256 rows the sum of the lengths
//   (b) dgram_scan_tiles    ONE workgroup turns the tile sums into exclusive tile bases, 1024 tiles per round of its loop, and
//                           stores the total behind the last row's offset
//   (c) dgram_unpack_copy   per tile: in-tile scan + tile base = the rows' offsets; then the rows are dealt to lane groups as in
//                           pack.  Here the source (row + 4) is aligned and the destination is at any phase: the bytes up to the
//                           first aligned dword of the destination and the bytes behind the last whole one go out as byte
//                           stores, the dwords between as dword stores of funnel-shifted pairs -- a dword store never covers a
//                           byte of the neighbouring datagram, which another lane group (or workgroup) writes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "internal.h"
#include "dgram_scan_dev.h"   // kThreads, kWaves, kScanPer, block_scan_excl, dgram_scan_tiles (shared with wire_ragged_dev.hip)
#include "../../include/ldpc_erasure_amd_datagrams.h"
#include "../../include/ldpc_erasure_amd_wire.h"

using namespace ldpc_amd;

namespace {

constexpr int kPre = LDPC_AMD_DGRAM_PREFIX_BYTES;
constexpr int kTile = kThreads;          // rows per tile of the unpack scan: one per thread
constexpr int64_t kMaxGrid = (int64_t)1 << 20;   // grid-stride loops cover the rest

inline unsigned grid_for(int64_t blocks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, kMaxGrid)); }

// ---- pack ------------------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(kThreads) void dgram_pack(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ off, int64_t N, int64_t R,
                                                       int W /* S / 4 */, uint32_t *__restrict__ source)
{
    constexpr int RPW = 64 / G, U = 4;
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G;
    const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kWaves;
    for (int64_t r0 = wave * RPW; r0 < R; r0 += nwaves * RPW) {
        const int64_t r = r0 + sub;
        if (r >= R) continue;
        uint64_t a = 0;
        uint32_t L = 0;
        if (r < N) {
            const int64_t o0 = off[r], o1 = off[r + 1];
            L = (uint32_t)(o1 - o0);
            if (L) a = (uint64_t)(uintptr_t)bytes + (uint64_t)o0;
        }
        const uint32_t ph = (uint32_t)(a & 3);
        const uint32_t *__restrict__ w = (const uint32_t *)(uintptr_t)(a - ph);
        const uint32_t nw = L ? (ph + L + 3) >> 2 : 0;   // the aligned dwords that contain a byte of the datagram
        uint32_t *__restrict__ dst = source + (size_t)r * (size_t)W;
        for (int j0 = 0; j0 < W; j0 += U * G) {
            uint32_t lo[U], hi[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int j = j0 + u * G + g;
                const uint32_t q = (uint32_t)(j - 1);   // data dword of this lane (j == 0: the prefix, q wraps and loads nothing)
                const bool in = j >= 1 && j < W;
                lo[u] = (in && q < nw) ? w[q] : 0u;
                hi[u] = (in && ph && q + 1 < nw) ? w[q + 1] : 0u;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int j = j0 + u * G + g;
                if (j >= W) continue;
                uint32_t v = L;
                if (j >= 1) {
                    const uint32_t first = 4u * (uint32_t)(j - 1);   // datagram byte of this dword's byte 0
                    v = __builtin_amdgcn_alignbyte(hi[u], lo[u], ph);
                    if (first >= L) v = 0;
                    else if (L - first < 4) v &= (1u << (8 * (L - first))) - 1u;
                }
                dst[j] = v;
            }
        }
    }
}

// ---- unpack ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dgram_unpack_lens(const uint8_t *__restrict__ frames, const uint8_t *__restrict__ erased, int64_t R,
                                                              int64_t T, int n, int k, int S, uint32_t *__restrict__ len, uint8_t *__restrict__ state,
                                                              unsigned long long *__restrict__ tilesum)
{
    __shared__ unsigned long long sw[kWaves];
    for (int64_t tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const int64_t r = tile * kTile + threadIdx.x;
        uint32_t L = 0;
        if (r < R) {
            const int64_t b = r / k, row = b * n + (r - b * k);
            int st = LDPC_AMD_DGRAM_LOST;
            if (!(erased && erased[row])) {
                L = *(const uint32_t *)(frames + (size_t)row * (size_t)S);
                st = L == 0 ? LDPC_AMD_DGRAM_FILLER : L > (uint32_t)(S - kPre) ? LDPC_AMD_DGRAM_MALFORMED : LDPC_AMD_DGRAM_DELIVERED;
                if (st != LDPC_AMD_DGRAM_DELIVERED) L = 0;
            }
            state[r] = (uint8_t)st;
            len[r] = L;
        }
        unsigned long long total;
        (void)block_scan_excl(L, sw, &total);
        if (threadIdx.x == 0) tilesum[tile] = total;
    }
}

template <int G>
__global__ __launch_bounds__(kThreads) void dgram_unpack_copy(const uint8_t *__restrict__ frames, int64_t R, int64_t T, int n, int k, int S,
                                                              const uint32_t *__restrict__ len, const unsigned long long *__restrict__ tilebase,
                                                              uint8_t *__restrict__ out, int64_t *__restrict__ offset_out)
{
    constexpr int RPW = 64 / G, U = 4;
    __shared__ unsigned long long sw[kWaves];
    __shared__ unsigned long long s_off[kTile];
    __shared__ uint32_t s_len[kTile];
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const int64_t rt = tile * kTile + threadIdx.x;
        const uint32_t Lt = rt < R ? len[rt] : 0u;
        unsigned long long total;
        const unsigned long long o = tilebase[tile] + block_scan_excl(Lt, sw, &total);
        if (rt < R) offset_out[rt] = (int64_t)o;
        s_off[threadIdx.x] = o;
        s_len[threadIdx.x] = Lt;
        __syncthreads();
        for (int i = wave * RPW + sub; i < kTile; i += kWaves * RPW) {
            const uint32_t L = s_len[i];
            if (!L) continue;   // (rows beyond R have length 0)
            const int64_t r = tile * kTile + i, b = r / k, row = b * n + (r - b * k);
            const uint8_t *__restrict__ sb = frames + (size_t)row * (size_t)S + kPre;
            const uint32_t *__restrict__ swd = (const uint32_t *)sb;
            uint8_t *__restrict__ d = out + s_off[i];
            uint32_t h = (4u - (uint32_t)((uintptr_t)d & 3)) & 3u;   // bytes up to the first aligned dword of the destination
            if (h > L) h = L;
            const uint32_t nd = (L - h) >> 2, t = L - h - 4u * nd;
            if ((uint32_t)g < h) d[g] = sb[g];
            if ((uint32_t)g < t) d[h + 4u * nd + g] = sb[h + 4u * nd + g];
            uint32_t *__restrict__ dw = (uint32_t *)(d + h);
            for (uint32_t q0 = 0; q0 < nd; q0 += U * G) {
                uint32_t lo[U], hi[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t q = q0 + u * G + g;
                    // with h != 0 the dword holds datagram bytes h + 4q .. h + 4q + 3 <= L - 1: source dword q + 1 lies inside the row
                    lo[u] = q < nd ? swd[q] : 0u;
                    hi[u] = (q < nd && h) ? swd[q + 1] : 0u;
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t q = q0 + u * G + g;
                    if (q < nd) dw[q] = __builtin_amdgcn_alignbyte(hi[u], lo[u], h);
                }
            }
        }
        // (the next round's first barrier, inside block_scan_excl, comes before s_off / s_len are rewritten)
    }
}

inline bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

inline bool symbol_ok(int S) { return S >= 8 && (S % 4) == 0; }

// lanes per row: 64 for rows of more than 32 dwords, else the power of two (at least 4: the head and tail bytes of unpack) that covers it
inline int lanes_per_row(int W)
{
    int g = 4;
    while (g < 64 && g < W) g <<= 1;
    return g;
}

// The first bad entry of offset[0..N], or -1: negative, decreasing, or a length above S - 4.
int64_t first_bad_offset(const int64_t *offset, int64_t N, int S)
{
    if (offset[0] < 0) return 0;
    for (int64_t i = 0; i < N; i++)
        if (offset[i + 1] < offset[i] || offset[i + 1] - offset[i] > (int64_t)(S - kPre)) return i;
    return -1;
}

}  // namespace

int64_t ldpc_amd_fec_dgram_wire_len(int64_t ndgrams, const int64_t *offset, int n, int k, int S, int32_t *wire_len)
{
    if (ndgrams < 0 || !offset || k < 1 || n < k || !symbol_ok(S)) return LDPC_AMD_EINVAL;
    if (first_bad_offset(offset, ndgrams, S) >= 0) return LDPC_AMD_EINVAL;
    const int64_t F = (ndgrams + k - 1) / k;
    if (F > (((int64_t)1 << 31) - 1) / n) return LDPC_AMD_EINVAL;   // F * n < 2^31
    if (wire_len)
        for (int64_t f = 0; f < F; f++) {
            int32_t *w = wire_len + f * n;
            for (int i = 0; i < k; i++) {
                const int64_t d = f * k + i;
                w[i] = (int32_t)(LDPC_AMD_FEC_HEADER_BYTES + kPre + (d < ndgrams ? offset[d + 1] - offset[d] : 0));
            }
            for (int i = k; i < n; i++) w[i] = LDPC_AMD_FEC_HEADER_BYTES + S;
        }
    return F * n;
}

int64_t ldpc_amd_fec_dgram_pack_dev(ldpc_amd_ctx *ctx, const uint8_t *bytes, const int64_t *offset, int64_t ndgrams, int k, int S, uint8_t *source)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (ndgrams < 0 || k < 1 || !offset) return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_pack_dev: need ndgrams >= 0, k >= 1 and an offset array");
    if (!symbol_ok(S)) return set_error(ctx, LDPC_AMD_EUNSUP, "fec_dgram_pack_dev: S must be a multiple of 4 that is at least 8 (got %d)", S);
    const int64_t bad = first_bad_offset(offset, ndgrams, S);
    if (bad >= 0) {
        if (offset[bad] < 0 || (bad < ndgrams && offset[bad + 1] < offset[bad]))
            return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_pack_dev: offsets must be non-negative and non-decreasing (index %lld)", (long long)bad);
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_pack_dev: datagram %lld has %lld bytes, a symbol of %d holds %d", (long long)bad,
                         (long long)(offset[bad + 1] - offset[bad]), S, S - kPre);
    }
    const int64_t F = (ndgrams + k - 1) / k;
    if (F > (((int64_t)1 << 31) - 1) / k)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_pack_dev: %lld frames of %d rows are not below 2^31 rows", (long long)F, k);
    if (ndgrams == 0) return 0;
    const int64_t R = F * k;
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nbytes = (size_t)(offset[ndgrams] - offset[0]), nsource = (size_t)R * (size_t)S;
    if (!source || !is_device_ptr(ctx, source) || (nbytes && (!bytes || !is_device_ptr(ctx, bytes))))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_pack_dev: bytes / source must be device pointers of device %d", ctx->device);
    if (((uintptr_t)source & 3) != 0) return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_pack_dev: source must be 4-byte aligned");
    if (nbytes && overlap(bytes + offset[0], nbytes, source, nsource)) return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_pack_dev: bytes and source overlap");
    // the offsets: through the context's pinned ring to the device (internal.h: PinnedRing)
    const size_t tab_bytes = sizeof(int64_t) * (size_t)(ndgrams + 1);
    int rc;
    if ((rc = scratch_reserve(ctx, ctx->dgram_off, tab_bytes))) return rc;
    void *stage = nullptr;
    size_t want = 0;
    if ((rc = pinned_ring_acquire(ctx, ctx->dgram_ring, tab_bytes, &stage, &want)))
        return rc == LDPC_AMD_ENOMEM ? set_error(ctx, LDPC_AMD_ENOMEM, "fec_dgram_pack_dev: no pinned memory for %zu offset bytes", want) : rc;
    memcpy(stage, offset, tab_bytes);
    LDPC_HIP_TRY(ctx, hipMemcpyAsync(ctx->dgram_off.p, stage, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pinned_ring_commit(ctx, ctx->dgram_ring))) return rc;
    const int W = S / 4, G = lanes_per_row(W);
    const dim3 grid(grid_for((R + (int64_t)kWaves * (64 / G) - 1) / ((int64_t)kWaves * (64 / G)))), block(kThreads);
    const int64_t *doff = (const int64_t *)ctx->dgram_off.p;
    uint32_t *dsrc = (uint32_t *)source;
    switch (G) {
    case 4: hipLaunchKernelGGL(dgram_pack<4>, grid, block, 0, ctx->stream, bytes, doff, ndgrams, R, W, dsrc); break;
    case 8: hipLaunchKernelGGL(dgram_pack<8>, grid, block, 0, ctx->stream, bytes, doff, ndgrams, R, W, dsrc); break;
    case 16: hipLaunchKernelGGL(dgram_pack<16>, grid, block, 0, ctx->stream, bytes, doff, ndgrams, R, W, dsrc); break;
    case 32: hipLaunchKernelGGL(dgram_pack<32>, grid, block, 0, ctx->stream, bytes, doff, ndgrams, R, W, dsrc); break;
    default: hipLaunchKernelGGL(dgram_pack<64>, grid, block, 0, ctx->stream, bytes, doff, ndgrams, R, W, dsrc); break;
    }
    LDPC_HIP_TRY(ctx, hipGetLastError());
    ctx->dgram_rows[0] = R;
    return F;
}

int ldpc_amd_fec_dgram_unpack_dev(ldpc_amd_ctx *ctx, const uint8_t *frames, const uint8_t *erased, int64_t nframes, int n, int k, int S,
                                  uint8_t *bytes_out, int64_t cap, int64_t *offset_out, uint8_t *state)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (nframes < 0 || k < 1 || n < k) return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_unpack_dev: need nframes >= 0 and 1 <= k <= n (n=%d k=%d)", n, k);
    if (!symbol_ok(S)) return set_error(ctx, LDPC_AMD_EUNSUP, "fec_dgram_unpack_dev: S must be a multiple of 4 that is at least 8 (got %d)", S);
    if (nframes > (((int64_t)1 << 31) - 1) / k)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_unpack_dev: %lld frames of %d rows are not below 2^31 rows", (long long)nframes, k);
    const int64_t R = nframes * k;
    if (cap < R * (int64_t)(S - kPre))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_unpack_dev: cap is %lld, %lld rows of %d bytes need %lld", (long long)cap, (long long)R, S - kPre,
                         (long long)(R * (int64_t)(S - kPre)));
    if (nframes == 0) return LDPC_AMD_OK;
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!frames || !bytes_out || !offset_out || !state || !is_device_ptr(ctx, frames) || !is_device_ptr(ctx, bytes_out) || !is_device_ptr(ctx, offset_out) ||
        !is_device_ptr(ctx, state) || (erased && !is_device_ptr(ctx, erased)))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_unpack_dev: frames / erased / bytes_out / offset_out / state must be device pointers of device %d",
                         ctx->device);
    if (((uintptr_t)frames & 3) != 0 || ((uintptr_t)offset_out & 7) != 0)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_unpack_dev: frames must be 4-byte and offset_out 8-byte aligned");
    {
        const void *p[5] = {frames, erased, bytes_out, offset_out, state};
        const size_t nb[5] = {(size_t)nframes * (size_t)n * (size_t)S, erased ? (size_t)nframes * (size_t)n : 0, (size_t)cap, sizeof(int64_t) * (size_t)(R + 1),
                              (size_t)R};
        for (int a = 0; a < 5; a++)
            for (int b = std::max(a + 1, 2); b < 5; b++)   // every pair with an output in it
                if (overlap(p[a], nb[a], p[b], nb[b])) return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_unpack_dev: an output overlaps an input or another output");
    }
    const int64_t T = (R + kTile - 1) / kTile;
    int rc;
    if ((rc = scratch_reserve(ctx, ctx->dgram_len, sizeof(unsigned long long) * (size_t)T + sizeof(uint32_t) * (size_t)R))) return rc;
    unsigned long long *tilesum = (unsigned long long *)ctx->dgram_len.p;
    uint32_t *len = (uint32_t *)(tilesum + T);
    const dim3 grid(grid_for(T)), block(kThreads);
    hipLaunchKernelGGL(dgram_unpack_lens, grid, block, 0, ctx->stream, frames, erased, R, T, n, k, S, len, state, tilesum);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(dgram_scan_tiles, dim3(1), block, 0, ctx->stream, tilesum, T, offset_out + R);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    switch (lanes_per_row(S / 4)) {
    case 4: hipLaunchKernelGGL(dgram_unpack_copy<4>, grid, block, 0, ctx->stream, frames, R, T, n, k, S, len, tilesum, bytes_out, offset_out); break;
    case 8: hipLaunchKernelGGL(dgram_unpack_copy<8>, grid, block, 0, ctx->stream, frames, R, T, n, k, S, len, tilesum, bytes_out, offset_out); break;
    case 16: hipLaunchKernelGGL(dgram_unpack_copy<16>, grid, block, 0, ctx->stream, frames, R, T, n, k, S, len, tilesum, bytes_out, offset_out); break;
    case 32: hipLaunchKernelGGL(dgram_unpack_copy<32>, grid, block, 0, ctx->stream, frames, R, T, n, k, S, len, tilesum, bytes_out, offset_out); break;
    default: hipLaunchKernelGGL(dgram_unpack_copy<64>, grid, block, 0, ctx->stream, frames, R, T, n, k, S, len, tilesum, bytes_out, offset_out); break;
    }
    LDPC_HIP_TRY(ctx, hipGetLastError());
    ctx->dgram_rows[1] = R;
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_dgram_info(ldpc_amd_ctx *ctx, int64_t info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_dgram_info: info must not be null");
    info[0] = (int64_t)(ctx->dgram_off.cap + ctx->dgram_len.cap);
    info[1] = (int64_t)ctx->dgram_ring.bytes();
    info[2] = ctx->dgram_rows[0];
    info[3] = ctx->dgram_rows[1];
    return LDPC_AMD_OK;
}
