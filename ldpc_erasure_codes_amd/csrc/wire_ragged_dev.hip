// wire_ragged_dev.hip -- the trimmed wire (include/ldpc_erasure_amd_wire_ragged.h): cut the packets of a fixed-stride packet array
// to the bytes that have to be sent and lay them back to back (TRIM), and put datagrams that lie back to back, with their
// boundaries in device memory, into the slots of a packet array, zero fill included (LAND).  Both are one bandwidth-bound pass
// with a byte funnel shift, the family of dgram_pack / dgram_unpack_copy (datagram_dev.hip).
//
// Reference: OpenCL/device/ldpc_erasure_encoder_VITA_in_UDP_out.cl:140-162 -- the sender takes every packet's length from the packet.
//
// A packet is 8 + S bytes = W dwords, W = (8 + S) / 4: dwords 0..1 the FEC header (symbol number = bytes 0..1, little-endian),
// dword 2 the length prefix L of a datagram symbol.
//
// TRIM, three launches (the shape of unpack), no workgroup ever waits for another:
//   (a) wire_trim_lens     per packet: its wire length from the header and the prefix; per tile of 256 packets the sum
//   (b) dgram_scan_tiles   ONE workgroup turns the tile sums into exclusive tile bases and stores the total behind the last offset
//   (c) wire_trim_copy     per tile: in-tile scan + tile base = the packets' offsets; then the packets are dealt to lane groups.
//                          The source (the packet) is 4-byte aligned, the destination at any byte phase: the bytes up to the first
//                          aligned dword of the destination and the bytes behind the last whole one go out as byte stores, the
//                          dwords between as dword stores of funnel-shifted pairs -- a dword store never covers a byte of the
//                          neighbouring datagram, which another lane group (or workgroup) writes.
// LAND, one launch (the shape of pack): the destination (the slot) is 4-byte aligned, the datagram starts at any byte phase ph of
// an aligned dword: a lane loads the two aligned dwords its four bytes straddle and funnel-shifts them by ph bytes; only aligned
// dwords that contain a byte of the datagram are loaded, bytes at or behind its length are masked to zero in the same store.  The
// boundaries are vetted per datagram in the kernel (they live on the device); of a rejected one nothing is loaded.  No barrier,
// no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "internal.h"
#include "dgram_scan_dev.h"   // kThreads, kWaves, block_scan_excl, dgram_scan_tiles
#include "../../include/ldpc_erasure_amd_datagrams.h"
#include "../../include/ldpc_erasure_amd_wire.h"
#include "../../include/ldpc_erasure_amd_wire_ragged.h"

using namespace ldpc_amd;

namespace {

constexpr int kHdr = LDPC_AMD_FEC_HEADER_BYTES;
constexpr int kPre = LDPC_AMD_DGRAM_PREFIX_BYTES;
constexpr int kTile = kThreads;          // packets per tile of the trim scan: one per thread
constexpr int64_t kMaxGrid = (int64_t)1 << 20;   // grid-stride loops cover the rest
constexpr int kMaxS = 1 << 30;
// dwords per lane and trip of a 64-lane group: 6 * 64 dwords = 1536 bytes, so that a packet of up to S = 1528 (an MTU's worth) is
// one trip -- all its loads in flight at once.  With 4 a packet of S = 1024 (258 dwords) took a second trip for its last 8 bytes,
// a whole memory latency with next to nothing in flight.
constexpr int kWideU = 6;

inline unsigned grid_for(int64_t blocks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, kMaxGrid)); }

// ---- trim ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void wire_trim_lens(const uint32_t *__restrict__ packets, int64_t P, int64_t T, int k, int W /* (8 + S) / 4 */,
                                                           uint32_t *__restrict__ len, unsigned long long *__restrict__ tilesum)
{
    __shared__ unsigned long long sw[kWaves];
    const uint32_t plen = 4u * (uint32_t)W, smax = plen - (uint32_t)(kHdr + kPre);   // S - 4
    for (int64_t tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const int64_t p = tile * kTile + threadIdx.x;
        uint32_t n = 0;
        if (p < P) {
            const uint32_t *__restrict__ h = packets + (size_t)p * (size_t)W;
            n = plen;
            if ((h[0] & 0xffffu) < (uint32_t)k) {   // a source row: dword 2 is its length prefix
                const uint32_t L = h[2];
                if (L <= smax) n = (uint32_t)(kHdr + kPre) + L;
            }
            len[p] = n;
        }
        unsigned long long total;
        (void)block_scan_excl(n, sw, &total);
        if (threadIdx.x == 0) tilesum[tile] = total;
    }
}

template <int G>
__global__ __launch_bounds__(kThreads) void wire_trim_copy(const uint8_t *__restrict__ packets, int64_t P, int64_t T, int W, const uint32_t *__restrict__ len,
                                                           const unsigned long long *__restrict__ tilebase, uint8_t *__restrict__ out,
                                                           int64_t *__restrict__ offset_out)
{
    constexpr int RPW = 64 / G, U = G == 64 ? kWideU : 4;
    __shared__ unsigned long long sw[kWaves];
    __shared__ unsigned long long s_off[kTile];
    __shared__ uint32_t s_len[kTile];
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const int64_t pt = tile * kTile + threadIdx.x;
        const uint32_t Lt = pt < P ? len[pt] : 0u;
        unsigned long long total;
        const unsigned long long o = tilebase[tile] + block_scan_excl(Lt, sw, &total);
        if (pt < P) offset_out[pt] = (int64_t)o;
        s_off[threadIdx.x] = o;
        s_len[threadIdx.x] = Lt;
        __syncthreads();
        for (int i = wave * RPW + sub; i < kTile; i += kWaves * RPW) {
            const uint32_t L = s_len[i];
            if (!L) continue;   // (only the packets beyond P have length 0)
            const uint8_t *__restrict__ sb = packets + (size_t)(tile * kTile + i) * (size_t)(4 * W);
            const uint32_t *__restrict__ swd = (const uint32_t *)sb;
            uint8_t *__restrict__ d = out + s_off[i];
            uint32_t h = (4u - (uint32_t)((uintptr_t)d & 3)) & 3u;   // bytes up to the first aligned dword of the destination (L >= 12 > h)
            const uint32_t nd = (L - h) >> 2, t = L - h - 4u * nd;
            if ((uint32_t)g < h) d[g] = sb[g];
            if ((uint32_t)g < t) d[h + 4u * nd + g] = sb[h + 4u * nd + g];
            uint32_t *__restrict__ dw = (uint32_t *)(d + h);
            for (uint32_t q0 = 0; q0 < nd; q0 += U * G) {
                uint32_t lo[U], hi[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t q = q0 + u * G + g;
                    // with h != 0 the dword holds packet bytes h + 4q .. h + 4q + 3 <= L - 1: source dword q + 1 lies inside the packet
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

// ---- land ------------------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(kThreads) void wire_land(const uint8_t *__restrict__ bytes, int64_t nbytes, const int64_t *__restrict__ off, int64_t P,
                                                      int W /* (8 + S) / 4 */, uint32_t *__restrict__ packets, uint8_t *__restrict__ state)
{
    constexpr int RPW = 64 / G, U = G == 64 ? kWideU : 4;
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G;
    const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kWaves;
    for (int64_t p0 = wave * RPW; p0 < P; p0 += nwaves * RPW) {
        const int64_t p = p0 + sub;
        if (p >= P) continue;
        const int64_t o0 = off[p], o1 = off[p + 1];
        bool ok = o0 >= 0 && o1 >= o0 && o1 <= nbytes;   // (then o1 - o0 does not overflow)
        if (ok) ok = o1 - o0 >= (int64_t)kHdr && o1 - o0 <= (int64_t)4 * W;
        const uint32_t L = ok ? (uint32_t)(o1 - o0) : 0u;
        const uint64_t a = ok ? (uint64_t)(uintptr_t)bytes + (uint64_t)o0 : 0;
        const uint32_t ph = (uint32_t)(a & 3);
        const uint32_t *__restrict__ w = (const uint32_t *)(uintptr_t)(a - ph);
        const uint32_t nw = L ? (ph + L + 3) >> 2 : 0;   // the aligned dwords that contain a byte of the datagram
        uint32_t *__restrict__ dst = packets + (size_t)p * (size_t)W;
        if (state && g == 0) state[p] = ok ? LDPC_AMD_WIRE_LANDED : LDPC_AMD_WIRE_REJECTED;
        for (int j0 = 0; j0 < W; j0 += U * G) {
            uint32_t lo[U], hi[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t j = (uint32_t)(j0 + u * G + g);
                lo[u] = j < nw ? w[j] : 0u;            // (nw <= W + 1, and j == W is beyond the slot: stored nowhere)
                hi[u] = (ph && j + 1 < nw) ? w[j + 1] : 0u;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int j = j0 + u * G + g;
                if (j >= W) continue;
                const uint32_t first = 4u * (uint32_t)j;   // datagram byte of this dword's byte 0
                uint32_t v = __builtin_amdgcn_alignbyte(hi[u], lo[u], ph);
                if (first >= L) v = 0;
                else if (L - first < 4) v &= (1u << (8 * (L - first))) - 1u;
                if (!ok) v = j < kHdr / 4 ? 0xFFFFFFFFu : 0u;   // a rejected slot: symbol 0xFFFF, which every receiver drops
                dst[j] = v;
            }
        }
    }
}

inline bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

inline bool symbol_ok(int S) { return S >= 8 && (S % 4) == 0 && S <= kMaxS; }

// lanes per packet: 64 for packets of more than 32 dwords, else the power of two (at least 4: the head and tail bytes of trim) that covers it
inline int lanes_per_row(int W)
{
    int g = 4;
    while (g < 64 && g < W) g <<= 1;
    return g;
}

}  // namespace

int ldpc_amd_fec_wire_trim_dev(ldpc_amd_ctx *ctx, const uint8_t *packets, int64_t npackets, int k, int S, uint8_t *bytes_out, int64_t cap,
                               int64_t *offset_out)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (npackets < 0 || npackets >= ((int64_t)1 << 31) || k < 1)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_trim_dev: need 0 <= npackets < 2^31 and k >= 1 (npackets=%lld k=%d)", (long long)npackets, k);
    if (!symbol_ok(S)) return set_error(ctx, LDPC_AMD_EUNSUP, "fec_wire_trim_dev: S must be a multiple of 4 that is at least 8 (got %d)", S);
    const int64_t P = npackets, plen = (int64_t)kHdr + S;
    if (cap < P * plen)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_trim_dev: cap is %lld, %lld packets of %lld bytes need %lld", (long long)cap, (long long)P,
                         (long long)plen, (long long)(P * plen));
    if (P == 0) return LDPC_AMD_OK;
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!packets || !bytes_out || !offset_out || !is_device_ptr(ctx, packets) || !is_device_ptr(ctx, bytes_out) || !is_device_ptr(ctx, offset_out))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_trim_dev: packets / bytes_out / offset_out must be device pointers of device %d", ctx->device);
    if (((uintptr_t)packets & 3) != 0 || ((uintptr_t)offset_out & 7) != 0)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_trim_dev: packets must be 4-byte and offset_out 8-byte aligned");
    {
        const size_t npk = (size_t)P * (size_t)plen, noff = sizeof(int64_t) * (size_t)(P + 1);
        if (overlap(packets, npk, bytes_out, (size_t)cap) || overlap(packets, npk, offset_out, noff) || overlap(bytes_out, (size_t)cap, offset_out, noff))
            return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_trim_dev: an output overlaps the input or the other output");
    }
    const int64_t T = (P + kTile - 1) / kTile;
    int rc;
    if ((rc = scratch_reserve(ctx, ctx->wire_len, sizeof(unsigned long long) * (size_t)T + sizeof(uint32_t) * (size_t)P))) return rc;
    unsigned long long *tilesum = (unsigned long long *)ctx->wire_len.p;
    uint32_t *len = (uint32_t *)(tilesum + T);
    const int W = (int)(plen / 4);
    const dim3 grid(grid_for(T)), block(kThreads);
    hipLaunchKernelGGL(wire_trim_lens, grid, block, 0, ctx->stream, (const uint32_t *)packets, P, T, k, W, len, tilesum);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(dgram_scan_tiles, dim3(1), block, 0, ctx->stream, tilesum, T, offset_out + P);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    switch (lanes_per_row(W)) {
    case 4: hipLaunchKernelGGL(wire_trim_copy<4>, grid, block, 0, ctx->stream, packets, P, T, W, len, tilesum, bytes_out, offset_out); break;
    case 8: hipLaunchKernelGGL(wire_trim_copy<8>, grid, block, 0, ctx->stream, packets, P, T, W, len, tilesum, bytes_out, offset_out); break;
    case 16: hipLaunchKernelGGL(wire_trim_copy<16>, grid, block, 0, ctx->stream, packets, P, T, W, len, tilesum, bytes_out, offset_out); break;
    case 32: hipLaunchKernelGGL(wire_trim_copy<32>, grid, block, 0, ctx->stream, packets, P, T, W, len, tilesum, bytes_out, offset_out); break;
    default: hipLaunchKernelGGL(wire_trim_copy<64>, grid, block, 0, ctx->stream, packets, P, T, W, len, tilesum, bytes_out, offset_out); break;
    }
    LDPC_HIP_TRY(ctx, hipGetLastError());
    ctx->wire_packets[0] = P;
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_wire_land_dev(ldpc_amd_ctx *ctx, const uint8_t *bytes, int64_t nbytes, const int64_t *offset, int64_t npackets, int S, uint8_t *packets,
                               uint8_t *state)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (npackets < 0 || npackets >= ((int64_t)1 << 31) || nbytes < 0)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_land_dev: need 0 <= npackets < 2^31 and nbytes >= 0 (npackets=%lld nbytes=%lld)", (long long)npackets,
                         (long long)nbytes);
    if (!symbol_ok(S)) return set_error(ctx, LDPC_AMD_EUNSUP, "fec_wire_land_dev: S must be a multiple of 4 that is at least 8 (got %d)", S);
    if (nbytes > 0 && !bytes) return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_land_dev: bytes is NULL with nbytes = %lld", (long long)nbytes);
    const int64_t P = npackets, plen = (int64_t)kHdr + S;
    if (P == 0) return LDPC_AMD_OK;
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!offset || !packets || !is_device_ptr(ctx, offset) || !is_device_ptr(ctx, packets) || (nbytes > 0 && !is_device_ptr(ctx, bytes)) ||
        (state && !is_device_ptr(ctx, state)))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_land_dev: bytes / offset / packets / state must be device pointers of device %d", ctx->device);
    if (((uintptr_t)packets & 3) != 0 || ((uintptr_t)offset & 7) != 0)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_land_dev: packets must be 4-byte and offset 8-byte aligned");
    {
        const size_t npk = (size_t)P * (size_t)plen, noff = sizeof(int64_t) * (size_t)(P + 1), nst = state ? (size_t)P : 0;
        if (overlap(packets, npk, bytes, (size_t)nbytes) || overlap(packets, npk, offset, noff) || overlap(packets, npk, state, nst) ||
            overlap(state, nst, bytes, (size_t)nbytes) || overlap(state, nst, offset, noff))
            return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_land_dev: packets or state overlaps another buffer");
    }
    const int W = (int)(plen / 4), G = lanes_per_row(W);
    const dim3 grid(grid_for((P + (int64_t)kWaves * (64 / G) - 1) / ((int64_t)kWaves * (64 / G)))), block(kThreads);
    uint32_t *dpk = (uint32_t *)packets;
    switch (G) {
    case 4: hipLaunchKernelGGL(wire_land<4>, grid, block, 0, ctx->stream, bytes, nbytes, offset, P, W, dpk, state); break;
    case 8: hipLaunchKernelGGL(wire_land<8>, grid, block, 0, ctx->stream, bytes, nbytes, offset, P, W, dpk, state); break;
    case 16: hipLaunchKernelGGL(wire_land<16>, grid, block, 0, ctx->stream, bytes, nbytes, offset, P, W, dpk, state); break;
    case 32: hipLaunchKernelGGL(wire_land<32>, grid, block, 0, ctx->stream, bytes, nbytes, offset, P, W, dpk, state); break;
    default: hipLaunchKernelGGL(wire_land<64>, grid, block, 0, ctx->stream, bytes, nbytes, offset, P, W, dpk, state); break;
    }
    LDPC_HIP_TRY(ctx, hipGetLastError());
    ctx->wire_packets[1] = P;
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_wire_ragged_info(ldpc_amd_ctx *ctx, int64_t info[3])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_wire_ragged_info: info must not be null");
    info[0] = (int64_t)ctx->wire_len.cap;
    info[1] = ctx->wire_packets[0];
    info[2] = ctx->wire_packets[1];
    return LDPC_AMD_OK;
}
