// link_dev.hip -- the link emulator (include/ldpc_erasure_amd_link.h): who arrives where and with what damage (PLAN), and the
// gathers that move the bytes, on a fixed-stride packet array (APPLY) and on a trimmed wire (APPLY_RAGGED).  The model -- the
// draws, the arrival order, the damage -- is stated in the header; tools/link_model.py is the same in numpy.
//
// PLAN, three launches, no atomics, no workgroup ever waits for another:
//   (a) link_plan_count    per tile of 256 packets: how many of its entries (two per packet: the original, a copy) exist
//   (b) dgram_scan_tiles   ONE workgroup turns the tile counts into exclusive tile bases; the total is *count_out
//   (c) link_plan_rank     a workgroup owns a tile.  The draws are pure functions of the index, so nothing per entry lives in
//                          global memory: the workgroup recomputes the key (0: does not exist, else 1 + arrival time relative to
//                          the window's start) of the entries of its tile and of a halo of window + 1 packets on either side into
//                          LDS, 8 bytes per packet.  time(e) lies in [i, i + 1 + window], so only entries of that neighbourhood can
//                          change places with an owned one:
//                              rank(e) = prefix(e) - #{e' < e, time(e') > time(e)} + #{e' > e, time(e') < time(e)}
//                          with prefix(e) = tile base + in-tile scan.  A thread ranks both entries of its packet in one sweep over
//                          the neighbourhood; consecutive threads read consecutive 8-byte words of LDS.  O(P * window) compares.
// APPLY, one launch: a lane group per arriving packet reads row src[q] and stores row q, in dwords -- or in 16-byte words where
// the rows and both arrays are 16-byte aligned --, the header patched and the payload flipped in registers.  The launch covers
// cap rows, the count is read on the device and the rest leaves at once.
// APPLY_RAGGED, three launches, the shape of trim (wire_ragged_dev.hip):
//   (a) link_ragged_lens   per arriving datagram: its length from the vetted boundaries of datagram src[q]; per tile the sum
//   (b) dgram_scan_tiles   the tile bases; the total goes to a scratch word
//   (c) link_ragged_copy   per tile: in-tile scan + tile base = offset_out; then the datagrams are dealt to lane groups.  Source
//                          and destination lie at any byte phase: the bytes up to the first aligned dword of the destination and
//                          those behind the last whole one go out as byte stores, the dwords between as dword stores of two
//                          aligned source dwords funnel-shifted by the phase of the source against the destination.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <set>
#include <unordered_map>

#include "internal.h"
#include "dgram_scan_dev.h"   // kThreads, kWaves, block_scan_excl, dgram_scan_tiles
#include "../../include/ldpc_erasure_amd_synth.h"
#include "../../include/ldpc_erasure_amd_wire.h"
#include "../../include/ldpc_erasure_amd_link.h"

using namespace ldpc_amd;

namespace {

constexpr int kHdr = LDPC_AMD_FEC_HEADER_BYTES;
constexpr int kTile = kThreads;                  // packets (plan) or arriving datagrams (apply_ragged) per tile: one per thread
constexpr int64_t kMaxGrid = (int64_t)1 << 20;   // grid-stride loops cover the rest
constexpr int kMaxS = 1 << 30;
constexpr int kWideU = 6;                        // dwords per lane and trip of a 64-lane group (wire_ragged_dev.hip has the reason)
constexpr uint32_t kFlip = 0x5A5A5A5Au;

inline unsigned grid_for(int64_t blocks) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, kMaxGrid)); }

// what the draws of a call depend on
struct LinkDraw {
    uint64_t seed, first;
    uint64_t t_dup, t_bad, t_badfor;   // thresholds: dup, bad_sym, bad_sym + foreign
    uint32_t wp1;                      // window + 1
    uint32_t flip;                     // LDPC_AMD_LINK_DUP_FLIP
};

// keys of packet i's two entries: 0 = does not exist, else 1 + time(e) - lo
__device__ inline uint2 entry_keys(const LinkDraw &d, const uint8_t *__restrict__ lost, int64_t i, int64_t lo)
{
    if (lost && lost[i]) return make_uint2(0u, 0u);
    const uint64_t g = d.first + (uint64_t)i;
    const uint32_t rel = (uint32_t)(i - lo) + 1u;
    const uint32_t d0 = (uint32_t)(((uint64_t)ldpc_synth_u32(d.seed, LDPC_AMD_LINK_STREAM_DELAY, 2 * g) * d.wp1) >> 32);
    uint32_t k1 = 0;
    if (ldpc_synth_bernoulli(d.seed, LDPC_AMD_LINK_STREAM_DUP, g, d.t_dup))
        k1 = rel + 1u + (uint32_t)(((uint64_t)ldpc_synth_u32(d.seed, LDPC_AMD_LINK_STREAM_DELAY, 2 * g + 1) * d.wp1) >> 32);
    return make_uint2(rel + d0, k1);
}

__device__ inline uint16_t entry_fate(const LinkDraw &d, int64_t i, int c)
{
    const uint64_t x = ldpc_synth_u64(d.seed, LDPC_AMD_LINK_STREAM_DAMAGE, 2 * (d.first + (uint64_t)i) + (uint64_t)c);
    const uint64_t r = x >> 32;
    uint32_t f = c ? (uint32_t)LDPC_AMD_LINK_COPY : 0u;
    if (r < d.t_bad) f |= LDPC_AMD_LINK_BADSYM;
    else if (r < d.t_badfor) f |= LDPC_AMD_LINK_FOREIGN | ((uint32_t)((x >> 8) & 0xff) << 8);
    if (c && d.flip) f |= LDPC_AMD_LINK_FLIPPED;
    return (uint16_t)f;
}

// ---- plan ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void link_plan_count(LinkDraw d, const uint8_t *__restrict__ lost, int64_t P, int64_t T,
                                                            unsigned long long *__restrict__ tilesum)
{
    __shared__ unsigned long long sw[kWaves];
    for (int64_t tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const int64_t i = tile * kTile + threadIdx.x;
        uint32_t n = 0;
        if (i < P && !(lost && lost[i])) n = 1u + (uint32_t)ldpc_synth_bernoulli(d.seed, LDPC_AMD_LINK_STREAM_DUP, d.first + (uint64_t)i, d.t_dup);
        unsigned long long total;
        (void)block_scan_excl(n, sw, &total);
        if (threadIdx.x == 0) tilesum[tile] = total;
    }
}

__global__ __launch_bounds__(kThreads) void link_plan_rank(LinkDraw d, const uint8_t *__restrict__ lost, int64_t P, int64_t T,
                                                           const unsigned long long *__restrict__ tilebase, int32_t *__restrict__ src_out,
                                                           uint16_t *__restrict__ fate_out, int64_t cap)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *sw = (unsigned long long *)smem;            // [kWaves]
    uint2 *keys = (uint2 *)(smem + sizeof(unsigned long long) * kWaves);   // [kTile + 2 * (window + 1)]
    const int64_t halo = (int64_t)d.wp1;
    for (int64_t tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const int64_t t0 = tile * kTile;
        const int64_t lo = std::max<int64_t>(0, t0 - halo), hi = std::min<int64_t>(P, t0 + kTile + halo);
        __syncthreads();   // the previous tile's sweeps are through
        for (int64_t j = lo + threadIdx.x; j < hi; j += kThreads) keys[j - lo] = entry_keys(d, lost, j, lo);
        __syncthreads();
        const int64_t i = t0 + threadIdx.x;
        const uint2 mine = i < P ? keys[i - lo] : make_uint2(0u, 0u);
        unsigned long long total;
        const unsigned long long base = tilebase[tile] + block_scan_excl((mine.x != 0) + (mine.y != 0), sw, &total);
        if (!mine.x) continue;   // lost (or beyond P): neither entry exists
        const uint32_t tA = mine.x, tB = mine.y, tA1 = tA - 1u, tB1 = tB - 1u;
        const uint2 *__restrict__ kp = keys + (i - lo);
        const int nl = (int)std::min<int64_t>(halo, i - lo), nr = (int)std::min<int64_t>(halo, hi - 1 - i);
        uint32_t lA = 0, lB = 0, rA = 0, rB = 0;
        // entries in front that arrive later (a key of 0, no entry, is never greater)
#pragma unroll 4
        for (int j = -nl; j < 0; j++) {
            const uint2 k = kp[j];
            lA += (k.x > tA) + (k.y > tA);
            lB += (k.x > tB) + (k.y > tB);
        }
        // entries behind that arrive earlier (0 - 1 wraps to the largest value: no entry is never earlier)
#pragma unroll 4
        for (int j = 1; j <= nr; j++) {
            const uint2 k = kp[j];
            rA += (k.x - 1u < tA1) + (k.y - 1u < tA1);
            rB += (k.x - 1u < tB1) + (k.y - 1u < tB1);
        }
        const uint32_t swap = tB && tB < tA;   // the copy overtakes its original
        const unsigned long long qA = base - lA + rA + swap;
        if (qA < (unsigned long long)cap) {
            src_out[qA] = (int32_t)i;
            fate_out[qA] = entry_fate(d, i, 0);
        }
        if (tB) {
            const unsigned long long qB = base + 1 - lB + rB - swap;
            if (qB < (unsigned long long)cap) {
                src_out[qB] = (int32_t)i;
                fate_out[qB] = entry_fate(d, i, 1);
            }
        }
    }
}

// ---- apply -----------------------------------------------------------------------------------------------------------------
__device__ inline int64_t clamp_count(const int64_t *__restrict__ count, int64_t cap) { return std::min<int64_t>(std::max<int64_t>(*count, 0), cap); }

__device__ inline uint32_t patch_header(uint32_t v, uint32_t f)
{
    if (f & LDPC_AMD_LINK_BADSYM) v |= 0x0000FFFFu;
    if (f & LDPC_AMD_LINK_FOREIGN) v = (v & 0xFF00FFFFu) | ((f >> 8) << 16);
    return v;
}

// vector j of a row: dwords 0 and 1 are the header
__device__ inline uint32_t patch_vec(uint32_t v, int j, uint32_t f, uint32_t flip) { return j < kHdr / 4 ? patch_header(v, f) : v ^ flip; }
__device__ inline uint4 patch_vec(uint4 v, int j, uint32_t f, uint32_t flip)
{
    if (j == 0) return make_uint4(patch_header(v.x, f), patch_header(v.y, f), v.z ^ flip, v.w ^ flip);
    return make_uint4(v.x ^ flip, v.y ^ flip, v.z ^ flip, v.w ^ flip);
}
__device__ inline uint32_t zero_vec(uint32_t) { return 0u; }
__device__ inline uint4 zero_vec(uint4) { return make_uint4(0u, 0u, 0u, 0u); }

template <typename V, int G>
__global__ __launch_bounds__(kThreads) void link_apply(const V *__restrict__ packets, int64_t P, int WV /* vectors per row */, const int32_t *__restrict__ src,
                                                       const uint16_t *__restrict__ fate, const int64_t *__restrict__ count, int64_t cap,
                                                       V *__restrict__ out, const int32_t *__restrict__ flow_of, int32_t *__restrict__ flow_of_out)
{
    // dwords: a packet of up to S = 1528 is one trip of a 64-lane group, all its loads in flight at once (as in trim)
    constexpr int RPW = 64 / G, U = (G == 64 && sizeof(V) == 4) ? kWideU : 4;
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G;
    const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kWaves;
    const int64_t Q = clamp_count(count, cap);
    for (int64_t q0 = wave * RPW; q0 < Q; q0 += nwaves * RPW) {
        const int64_t q = q0 + sub;
        if (q >= Q) continue;
        const int64_t s = src[q];
        const bool ok = s >= 0 && s < P;
        // a source outside the array: the BADSYM slot of zeros, whatever the fate says
        const uint32_t f = ok ? (uint32_t)fate[q] : (uint32_t)LDPC_AMD_LINK_BADSYM;
        const uint32_t flip = (f & LDPC_AMD_LINK_FLIPPED) ? kFlip : 0u;
        const V *__restrict__ row = packets + (size_t)(ok ? s : 0) * (size_t)WV;
        V *__restrict__ dst = out + (size_t)q * (size_t)WV;
        if (flow_of_out && g == 0) flow_of_out[q] = ok ? flow_of[s] : -1;
        for (int j0 = 0; j0 < WV; j0 += U * G) {
            V v[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int j = j0 + u * G + g;
                v[u] = (ok && j < WV) ? row[j] : zero_vec(V{});
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int j = j0 + u * G + g;
                if (j < WV) dst[j] = patch_vec(v[u], j, f, flip);
            }
        }
    }
}

// ---- apply, ragged ---------------------------------------------------------------------------------------------------------
// length of datagram s of the input (0: bad boundaries, shorter than a header, or no such datagram) and where it starts
__device__ inline uint64_t ragged_len(const int64_t *__restrict__ off, int64_t nbytes, int64_t P, int64_t s, int64_t *start)
{
    *start = 0;
    if (s < 0 || s >= P) return 0;
    const int64_t o0 = off[s], o1 = off[s + 1];
    if (!(o0 >= 0 && o1 >= o0 && o1 <= nbytes)) return 0;   // (then o1 - o0 does not overflow)
    if (o1 - o0 < (int64_t)kHdr) return 0;
    *start = o0;
    return (uint64_t)(o1 - o0);
}

__global__ __launch_bounds__(kThreads) void link_ragged_lens(const int64_t *__restrict__ off, int64_t nbytes, int64_t P, const int32_t *__restrict__ src,
                                                             const int64_t *__restrict__ count, int64_t cap, int64_t T,
                                                             unsigned long long *__restrict__ tilesum)
{
    __shared__ unsigned long long sw[kWaves];
    const int64_t Q = clamp_count(count, cap);
    for (int64_t tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const int64_t q = tile * kTile + threadIdx.x;
        int64_t start;
        const unsigned long long n = q < Q ? ragged_len(off, nbytes, P, src[q], &start) : 0ull;
        unsigned long long total;
        (void)block_scan_excl(n, sw, &total);
        if (threadIdx.x == 0) tilesum[tile] = total;
    }
}

// byte idx of a datagram under the fate f
__device__ inline uint32_t patch_byte(uint32_t b, uint64_t idx, uint32_t f)
{
    if (idx >= (uint64_t)kHdr) return (f & LDPC_AMD_LINK_FLIPPED) ? b ^ 0x5Au : b;
    const uint32_t r = (uint32_t)idx & 3u;
    if (r < 2u) return (f & LDPC_AMD_LINK_BADSYM) ? 0xFFu : b;
    if (r == 2u) return (f & LDPC_AMD_LINK_FOREIGN) ? (f >> 8) & 0xFFu : b;
    return b;
}

// the dword that holds the datagram's bytes b0 .. b0 + 3
__device__ inline uint32_t patch_dword(uint32_t v, uint64_t b0, uint32_t f)
{
    if (b0 >= (uint64_t)kHdr) return (f & LDPC_AMD_LINK_FLIPPED) ? v ^ kFlip : v;
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) r |= patch_byte((v >> (8 * b)) & 0xFFu, b0 + b, f) << (8 * b);
    return r;
}

template <int G>
__global__ __launch_bounds__(kThreads) void link_ragged_copy(const uint8_t *__restrict__ bytes, int64_t nbytes, const int64_t *__restrict__ off, int64_t P,
                                                             const int32_t *__restrict__ src, const uint16_t *__restrict__ fate,
                                                             const int64_t *__restrict__ count, int64_t cap, int64_t T,
                                                             const unsigned long long *__restrict__ tilebase, uint8_t *__restrict__ out, int64_t bytes_cap,
                                                             int64_t *__restrict__ offset_out, int64_t *__restrict__ total_out)
{
    constexpr int RPW = 64 / G, U = G == 64 ? kWideU : 4;
    __shared__ unsigned long long sw[kWaves];
    __shared__ unsigned long long s_off[kTile], s_len[kTile];
    __shared__ int64_t s_start[kTile];
    __shared__ uint32_t s_fate[kTile];
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G, wave = threadIdx.x >> 6;
    const int64_t Q = clamp_count(count, cap);
    for (int64_t tile = blockIdx.x; tile < T; tile += gridDim.x) {
        if (tile * kTile > Q) break;   // (the tile that holds entry Q stores the total)
        const int64_t qt = tile * kTile + threadIdx.x;
        int64_t start = 0;
        const unsigned long long Lt = qt < Q ? ragged_len(off, nbytes, P, src[qt], &start) : 0ull;
        unsigned long long total;
        const unsigned long long o = tilebase[tile] + block_scan_excl(Lt, sw, &total);
        if (qt <= Q) offset_out[qt] = (int64_t)o;
        if (qt == Q && total_out) *total_out = (int64_t)o;
        s_off[threadIdx.x] = o;
        s_len[threadIdx.x] = o + Lt <= (unsigned long long)bytes_cap ? Lt : 0ull;   // a datagram that would end beyond the buffer is not written
        s_start[threadIdx.x] = start;
        s_fate[threadIdx.x] = Lt ? (uint32_t)fate[qt] : 0u;
        __syncthreads();
        for (int i = wave * RPW + sub; i < kTile; i += kWaves * RPW) {
            const uint64_t L = s_len[i];
            if (!L) continue;
            const uint32_t f = s_fate[i];
            const uint8_t *__restrict__ sb = bytes + s_start[i];
            uint8_t *__restrict__ d = out + s_off[i];
            const uint32_t h = (4u - (uint32_t)((uintptr_t)d & 3)) & 3u;   // bytes up to the first aligned dword of the destination (L >= 8 > h)
            const uint64_t nd = (L - h) >> 2;
            const uint32_t t = (uint32_t)((L - h) & 3u);
            if ((uint32_t)g < h) d[g] = (uint8_t)patch_byte(sb[g], (uint64_t)g, f);
            if ((uint32_t)g < t) {
                const uint64_t idx = h + 4u * nd + (uint32_t)g;
                d[idx] = (uint8_t)patch_byte(sb[idx], idx, f);
            }
            // destination dword q holds the datagram's bytes h + 4q .. h + 4q + 3; they straddle two aligned dwords of the source
            const uint64_t a = (uint64_t)(uintptr_t)(sb + h);
            const uint32_t ph = (uint32_t)(a & 3);
            const uint32_t *__restrict__ w = (const uint32_t *)(uintptr_t)(a - ph);
            uint32_t *__restrict__ dw = (uint32_t *)(d + h);
            for (uint64_t q0 = 0; q0 < nd; q0 += U * G) {
                uint32_t lo[U], hi[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint64_t q = q0 + (uint64_t)(u * G + g);
                    // with ph != 0 the last byte of the dword, datagram byte h + 4q + 3 <= L - 1, lies in source dword q + 1
                    lo[u] = q < nd ? w[q] : 0u;
                    hi[u] = (q < nd && ph) ? w[q + 1] : 0u;
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint64_t q = q0 + (uint64_t)(u * G + g);
                    if (q < nd) dw[q] = patch_dword(__builtin_amdgcn_alignbyte(hi[u], lo[u], ph), h + 4u * q, f);
                }
            }
        }
        // (the next round's first barrier, inside block_scan_excl, comes before the s_ arrays are rewritten)
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

struct Span {
    const void *p;
    size_t n;
};

// an output must not overlap any input or another output
template <size_t NO, size_t NI>
bool any_overlap(const Span (&outs)[NO], const Span (&ins)[NI])
{
    for (size_t a = 0; a < NO; a++) {
        for (size_t b = a + 1; b < NO; b++)
            if (overlap(outs[a].p, outs[a].n, outs[b].p, outs[b].n)) return true;
        for (size_t b = 0; b < NI; b++)
            if (overlap(outs[a].p, outs[a].n, ins[b].p, ins[b].n)) return true;
    }
    return false;
}

inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// lanes per row: 64 for rows of more than 32 vectors, else the power of two (at least 4: the head and tail bytes of the ragged copy) that covers it
inline int lanes_per_row(int64_t W)
{
    int g = 4;
    while (g < 64 && g < W) g <<= 1;
    return g;
}

// The context's structure belongs to the other translation units and is not changed for the link: what the link keeps per context
// -- its scratch (tile sums) and the counters of ldpc_amd_fec_link_info -- lives in this table.  ldpc_amd_cleanup does not know it,
// so a block is held until the process ends; a context created at the address of a closed one takes the block over (device
// memory stays valid, and every call orders its kernels on its own stream), unless it is of another device.
struct LinkState {
    Scratch scratch;
    int device = -1;
    int64_t packets[3] = {0, 0, 0};   // of the last plan, apply, apply_ragged
};
std::mutex g_mu;
std::unordered_map<const ldpc_amd_ctx *, LinkState> g_state;
std::set<int> g_lds_set;   // devices on which link_plan_rank's dynamic LDS limit has been raised

LinkState &link_state(const ldpc_amd_ctx *ctx)
{
    std::lock_guard<std::mutex> lk(g_mu);
    LinkState &st = g_state[ctx];   // (references into an unordered_map stay valid)
    if (st.device != ctx->device) {
        st = LinkState{};
        st.device = ctx->device;
    }
    return st;
}

constexpr size_t kPlanLdsMax = sizeof(unsigned long long) * kWaves + sizeof(uint2) * (size_t)(kTile + 2 * (LDPC_AMD_LINK_MAX_WINDOW + 1));

hipError_t raise_plan_lds(int device)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_lds_set.count(device)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void *)link_plan_rank, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPlanLdsMax);
    if (e == hipSuccess) g_lds_set.insert(device);
    return e;
}

inline bool prob_ok(double p) { return p >= 0.0 && p <= 1.0; }   // (false for a NaN)

}  // namespace

int ldpc_amd_fec_link_plan_dev(ldpc_amd_ctx *ctx, const ldpc_amd_link_params *pr, int64_t npackets, const uint8_t *lost, int32_t *src_out,
                               uint16_t *fate_out, int64_t cap, int64_t *count_out)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!pr) return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_plan_dev: params must not be null");
    const int64_t P = npackets;
    if (P < 0 || P >= ((int64_t)1 << 30))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_plan_dev: need 0 <= npackets < 2^30 (got %lld)", (long long)P);
    if (cap < 2 * P)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_plan_dev: cap is %lld, %lld packets need 2 * npackets = %lld", (long long)cap, (long long)P,
                         (long long)(2 * P));
    if (pr->window < 0 || pr->window > LDPC_AMD_LINK_MAX_WINDOW)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_plan_dev: window must lie in 0 .. %d (got %d)", LDPC_AMD_LINK_MAX_WINDOW, (int)pr->window);
    if (!prob_ok(pr->dup) || !prob_ok(pr->bad_sym) || !prob_ok(pr->foreign) || !(pr->bad_sym + pr->foreign <= 1.0))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_plan_dev: dup, bad_sym and foreign must lie in [0, 1] and bad_sym + foreign <= 1 (got %g %g %g)",
                         pr->dup, pr->bad_sym, pr->foreign);
    if (pr->flags & ~LDPC_AMD_LINK_DUP_FLIP) return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_plan_dev: unknown flags 0x%x", (unsigned)pr->flags);
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!count_out || !is_device_ptr(ctx, count_out) || (lost && P > 0 && !is_device_ptr(ctx, lost)) ||
        (P > 0 && (!src_out || !fate_out || !is_device_ptr(ctx, src_out) || !is_device_ptr(ctx, fate_out))))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_plan_dev: lost / src_out / fate_out / count_out must be device pointers of device %d", ctx->device);
    if (!aligned(src_out, 4) || !aligned(fate_out, 2) || !aligned(count_out, 8))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_plan_dev: src_out must be 4-byte, fate_out 2-byte and count_out 8-byte aligned");
    {
        const Span outs[] = {{src_out, sizeof(int32_t) * (size_t)cap}, {fate_out, sizeof(uint16_t) * (size_t)cap}, {count_out, sizeof(int64_t)}};
        const Span ins[] = {{lost, (size_t)P}};
        if (any_overlap(outs, ins)) return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_plan_dev: an output overlaps lost or another output");
    }
    LinkState &st = link_state(ctx);
    if (P == 0) {
        LDPC_HIP_TRY(ctx, hipMemsetAsync(count_out, 0, sizeof(int64_t), ctx->stream));
        st.packets[0] = 0;
        return LDPC_AMD_OK;
    }
    LinkDraw d;
    d.seed = pr->seed;
    d.first = pr->first;
    d.t_dup = ldpc_synth_threshold(pr->dup);
    d.t_bad = ldpc_synth_threshold(pr->bad_sym);
    d.t_badfor = d.t_bad + ldpc_synth_threshold(pr->foreign);
    d.wp1 = (uint32_t)pr->window + 1u;
    d.flip = (pr->flags & LDPC_AMD_LINK_DUP_FLIP) ? 1u : 0u;
    const int64_t T = (P + kTile - 1) / kTile;
    int rc;
    if ((rc = scratch_reserve(ctx, st.scratch, sizeof(unsigned long long) * (size_t)(T + 1)))) return rc;
    unsigned long long *tilesum = (unsigned long long *)st.scratch.p;
    const size_t lds = sizeof(unsigned long long) * kWaves + sizeof(uint2) * (size_t)(kTile + 2 * (size_t)d.wp1);
    if (lds > 48 * 1024) LDPC_HIP_TRY(ctx, raise_plan_lds(ctx->device));
    const dim3 grid(grid_for(T)), block(kThreads);
    hipLaunchKernelGGL(link_plan_count, grid, block, 0, ctx->stream, d, lost, P, T, tilesum);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(dgram_scan_tiles, dim3(1), block, 0, ctx->stream, tilesum, T, count_out);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(link_plan_rank, grid, block, lds, ctx->stream, d, lost, P, T, tilesum, src_out, fate_out, cap);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    st.packets[0] = P;
    return LDPC_AMD_OK;
}

template <typename V>
static void launch_apply(ldpc_amd_ctx *ctx, int G, dim3 grid, const uint8_t *packets, int64_t P, int WV, const int32_t *src, const uint16_t *fate,
                         const int64_t *count, int64_t cap, uint8_t *out, const int32_t *flow_of, int32_t *flow_of_out)
{
    const dim3 block(kThreads);
    const V *in = (const V *)packets;
    V *o = (V *)out;
    switch (G) {
    case 4: hipLaunchKernelGGL((link_apply<V, 4>), grid, block, 0, ctx->stream, in, P, WV, src, fate, count, cap, o, flow_of, flow_of_out); break;
    case 8: hipLaunchKernelGGL((link_apply<V, 8>), grid, block, 0, ctx->stream, in, P, WV, src, fate, count, cap, o, flow_of, flow_of_out); break;
    case 16: hipLaunchKernelGGL((link_apply<V, 16>), grid, block, 0, ctx->stream, in, P, WV, src, fate, count, cap, o, flow_of, flow_of_out); break;
    case 32: hipLaunchKernelGGL((link_apply<V, 32>), grid, block, 0, ctx->stream, in, P, WV, src, fate, count, cap, o, flow_of, flow_of_out); break;
    default: hipLaunchKernelGGL((link_apply<V, 64>), grid, block, 0, ctx->stream, in, P, WV, src, fate, count, cap, o, flow_of, flow_of_out); break;
    }
}

int ldpc_amd_fec_link_apply_dev(ldpc_amd_ctx *ctx, const uint8_t *packets, int64_t npackets, int S, const int32_t *src, const uint16_t *fate,
                                const int64_t *count, int64_t cap, uint8_t *packets_out, const int32_t *flow_of, int32_t *flow_of_out)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    const int64_t P = npackets, lim = (int64_t)1 << 31;
    if (P < 0 || P >= lim || cap < 0 || cap >= lim)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_dev: need 0 <= npackets < 2^31 and 0 <= cap < 2^31 (npackets=%lld cap=%lld)", (long long)P,
                         (long long)cap);
    if (!(S >= 8 && (S % 4) == 0 && S <= kMaxS))
        return set_error(ctx, LDPC_AMD_EUNSUP, "fec_link_apply_dev: S must be a multiple of 4 that is at least 8 (got %d)", S);
    if ((flow_of == nullptr) != (flow_of_out == nullptr))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_dev: flow_of and flow_of_out must both be given or both be NULL");
    if (cap == 0) return LDPC_AMD_OK;
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((P > 0 && (!packets || !is_device_ptr(ctx, packets))) || !src || !fate || !count || !packets_out || !is_device_ptr(ctx, src) ||
        !is_device_ptr(ctx, fate) || !is_device_ptr(ctx, count) || !is_device_ptr(ctx, packets_out) ||
        (flow_of && ((P > 0 && !is_device_ptr(ctx, flow_of)) || !is_device_ptr(ctx, flow_of_out))))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_dev: packets / src / fate / count / packets_out / flow_of / flow_of_out must be device pointers of device %d",
                         ctx->device);
    if (!aligned(packets, 4) || !aligned(packets_out, 4) || !aligned(src, 4) || !aligned(fate, 2) || !aligned(count, 8) || !aligned(flow_of, 4) ||
        !aligned(flow_of_out, 4))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_dev: packets, packets_out, src and the flow arrays must be 4-byte, fate 2-byte and count 8-byte aligned");
    const int64_t plen = (int64_t)kHdr + S;
    {
        const Span outs[] = {{packets_out, (size_t)cap * (size_t)plen}, {flow_of_out, sizeof(int32_t) * (size_t)cap}};
        const Span ins[] = {{packets, (size_t)P * (size_t)plen}, {src, sizeof(int32_t) * (size_t)cap}, {fate, sizeof(uint16_t) * (size_t)cap},
                            {count, sizeof(int64_t)}, {flow_of, sizeof(int32_t) * (size_t)P}};
        if (any_overlap(outs, ins)) return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_dev: an output overlaps an input or the other output");
    }
    // 16-byte words where every row of both arrays starts on a 16-byte boundary, else dwords
    const bool wide = (plen % 16) == 0 && aligned(packets, 16) && aligned(packets_out, 16);
    const int WV = (int)(plen / (wide ? 16 : 4)), G = lanes_per_row(WV);
    const dim3 grid(grid_for((cap + (int64_t)kWaves * (64 / G) - 1) / ((int64_t)kWaves * (64 / G))));
    if (wide) launch_apply<uint4>(ctx, G, grid, packets, P, WV, src, fate, count, cap, packets_out, flow_of, flow_of_out);
    else launch_apply<uint32_t>(ctx, G, grid, packets, P, WV, src, fate, count, cap, packets_out, flow_of, flow_of_out);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    link_state(ctx).packets[1] = P;
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_link_apply_ragged_dev(ldpc_amd_ctx *ctx, const uint8_t *bytes, int64_t nbytes, const int64_t *offset, int64_t npackets, const int32_t *src,
                                       const uint16_t *fate, const int64_t *count, int64_t cap, uint8_t *bytes_out, int64_t bytes_cap, int64_t *offset_out,
                                       int64_t *total_out)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    const int64_t P = npackets, lim = (int64_t)1 << 31;
    if (P < 0 || P >= lim || cap < 0 || cap >= lim || nbytes < 0 || bytes_cap < 0)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_ragged_dev: need 0 <= npackets, cap < 2^31 and nbytes, bytes_cap >= 0 (npackets=%lld cap=%lld nbytes=%lld bytes_cap=%lld)",
                         (long long)P, (long long)cap, (long long)nbytes, (long long)bytes_cap);
    if (nbytes > (int64_t)(INT64_MAX / 2) || bytes_cap < 2 * nbytes)
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_ragged_dev: bytes_cap is %lld, %lld bytes need 2 * nbytes = %lld", (long long)bytes_cap,
                         (long long)nbytes, (long long)(2 * nbytes));
    if (nbytes > 0 && !bytes) return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_ragged_dev: bytes is NULL with nbytes = %lld", (long long)nbytes);
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!offset || !count || !offset_out || !is_device_ptr(ctx, offset) || !is_device_ptr(ctx, count) || !is_device_ptr(ctx, offset_out) ||
        (cap > 0 && (!src || !fate || !is_device_ptr(ctx, src) || !is_device_ptr(ctx, fate))) || (nbytes > 0 && !is_device_ptr(ctx, bytes)) ||
        (bytes_cap > 0 && (!bytes_out || !is_device_ptr(ctx, bytes_out))) || (total_out && !is_device_ptr(ctx, total_out)))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_ragged_dev: bytes / offset / src / fate / count / bytes_out / offset_out / total_out must be device pointers of device %d",
                         ctx->device);
    if (!aligned(src, 4) || !aligned(fate, 2) || !aligned(offset, 8) || !aligned(count, 8) || !aligned(offset_out, 8) || !aligned(total_out, 8))
        return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_ragged_dev: src must be 4-byte, fate 2-byte, offset, count, offset_out and total_out 8-byte aligned");
    {
        const Span outs[] = {{bytes_out, (size_t)bytes_cap}, {offset_out, sizeof(int64_t) * (size_t)(cap + 1)}, {total_out, sizeof(int64_t)}};
        const Span ins[] = {{bytes, (size_t)nbytes}, {offset, sizeof(int64_t) * (size_t)(P + 1)}, {src, sizeof(int32_t) * (size_t)cap},
                            {fate, sizeof(uint16_t) * (size_t)cap}, {count, sizeof(int64_t)}};
        if (any_overlap(outs, ins)) return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_apply_ragged_dev: an output overlaps an input or another output");
    }
    LinkState &st = link_state(ctx);
    const int64_t T = (cap + 1 + kTile - 1) / kTile;   // entry Q <= cap of offset_out belongs to a tile too
    int rc;
    if ((rc = scratch_reserve(ctx, st.scratch, sizeof(unsigned long long) * (size_t)(T + 1)))) return rc;
    unsigned long long *tilesum = (unsigned long long *)st.scratch.p;
    int64_t *total = (int64_t *)(tilesum + T);   // (the copy takes the total from its own scan)
    const int G = lanes_per_row(P > 0 ? nbytes / P / 4 : 0);   // by the mean length of a datagram
    const dim3 grid(grid_for(T)), block(kThreads);
    hipLaunchKernelGGL(link_ragged_lens, grid, block, 0, ctx->stream, offset, nbytes, P, src, count, cap, T, tilesum);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(dgram_scan_tiles, dim3(1), block, 0, ctx->stream, tilesum, T, total);
    LDPC_HIP_TRY(ctx, hipGetLastError());
#define LINK_RAGGED_COPY(GG)                                                                                                                       \
    hipLaunchKernelGGL(link_ragged_copy<GG>, grid, block, 0, ctx->stream, bytes, nbytes, offset, P, src, fate, count, cap, T, tilesum, bytes_out, \
                       bytes_cap, offset_out, total_out)
    switch (G) {
    case 4: LINK_RAGGED_COPY(4); break;
    case 8: LINK_RAGGED_COPY(8); break;
    case 16: LINK_RAGGED_COPY(16); break;
    case 32: LINK_RAGGED_COPY(32); break;
    default: LINK_RAGGED_COPY(64); break;
    }
#undef LINK_RAGGED_COPY
    LDPC_HIP_TRY(ctx, hipGetLastError());
    st.packets[2] = P;
    return LDPC_AMD_OK;
}

int ldpc_amd_fec_link_info(ldpc_amd_ctx *ctx, int64_t info[4])
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (!info) return set_error(ctx, LDPC_AMD_EINVAL, "fec_link_info: info must not be null");
    const LinkState &st = link_state(ctx);
    info[0] = (int64_t)st.scratch.cap;
    info[1] = st.packets[0];
    info[2] = st.packets[1];
    info[3] = st.packets[2];
    return LDPC_AMD_OK;
}
