// rs_wire_dev.hip -- the Reed-Solomon sender of the FEC wire (include/ldpc_erasure_amd_rs_wire.h): source blocks -> wire packets in one
// kernel, every block placed and numbered by the 16-byte descriptor the descriptor-driven senders of wire_dev.hip use.
//
// codeword = source * [I | P] (Matlab/Test_My_RS_Decode.m:48).  rs_encode_kernel (rs_kernels.inc) forms every parity row by reading all k
// source rows again: (n-k) k row reads per block, and the codewords then go through a packetiser.  Here, as in the streaming phase of
// rs_decode_packets_kernel: one WAVEFRONT per (block, 256-byte slice of its symbols), one dword per lane.  Every source
// row is read from HBM once, stored to the payload of its packet, its three byte-select index words are built once, and it is multiplied
// into the n-k parity accumulators, which live in registers:  acc[q] ^= P[t][q] * v.  Then the accumulators are stored to the parity
// packets.  The coefficient of a product is the same for the whole wavefront: it comes out of a scalar register (the coefficients of a
// source row are scalar dword loads from a padded copy of P, four to a dword), and its multiply table -- 5 dwords -- arrives by scalar
// loads too.  Per product and dword that leaves the three byte selects, the two xors and two moves on the vector ALU (a byte select
// takes its 8-byte table half from two scalar registers, and an instruction of gfx950 reads one): DESIGN.md 4.4b has the numbers.
//
// GF(256) tables: csrc/gf256_dev.h defines its __constant__ tables for exactly one device unit (kernels.hip).  This unit does not include
// it: the multiply table is a device buffer of the context (ldpc_amd_ctx::rsw_tab, filled once from build_mul3_tables), passed to the
// kernel as a pointer, and the four inline functions of the packed multiply are restated below.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <array>

#include "fec_header_dev.h"
#include "internal.h"

using namespace ldpc_amd;

namespace {

constexpr int kHdr = 8;      // LDPC_AMD_FEC_HEADER_BYTES
constexpr int kSlice = 256;  // bytes of every row per wavefront: one dword per lane
constexpr int kWaves = 4;    // wavefronts per workgroup
constexpr int kQMax = 64;    // accumulators of one pass over the source rows

// one block's place on the wire: row j is packet first + j * stride, its header class = hdr >> 8, block = hdr & 0xff (TxFrameDesc)
struct RswDesc {
    uint64_t first;
    uint32_t stride;
    uint32_t hdr;
};
static_assert(sizeof(RswDesc) == 16, "the senders stage 16-byte descriptors");

// memory that no kernel of the launch writes, read at wave-uniform addresses: the constant address space makes the loads scalar loads
typedef __attribute__((address_space(4))) const uint32_t cu32;
__device__ __forceinline__ cu32 *as_const(const void *p) { return (cu32 *)(uintptr_t)p; }

// ---- the packed multiply (gf256_dev.h): c*x = c*(x & 7) ^ c*((x >> 3 & 7) << 3) ^ c*((x >> 6) << 6), the 8 + 8 + 4 partial products of
// the coefficient in five dwords, each term one v_perm_b32 byte select
struct MulTab {
    uint32_t t0, t1, t2, t3, t4;
};
struct Sel3 {
    uint32_t s0, s1, s2;
};
__device__ __forceinline__ MulTab load_multab(cu32 *mul3, uint32_t c)   // c wave-uniform
{
    cu32 *p = mul3 + c * 8;
    return MulTab{p[0], p[1], p[2], p[3], p[4]};
}
__device__ __forceinline__ Sel3 gfsel(uint32_t x) { return Sel3{x & 0x07070707u, (x >> 3) & 0x07070707u, (x >> 6) & 0x03030303u}; }
__device__ __forceinline__ uint32_t gfmac4_sel(uint32_t acc, const MulTab &t, const Sel3 &s)   // acc ^ c * x
{
    return __builtin_amdgcn_bitop3_b32(acc, __builtin_amdgcn_perm(t.t1, t.t0, s.s0), __builtin_amdgcn_perm(t.t3, t.t2, s.s1), 0x96) ^
           __builtin_amdgcn_perm(t.t4, t.t4, s.s2);
}

// ---- the coefficients as the kernel reads them: coef[t][q] = P[t][q] = g[t][k + q], q < R, rows padded with zeros to qtot bytes (a
// multiple of the pass width, so of 4): a zero coefficient selects the all-zero table and adds nothing
__global__ __launch_bounds__(256) void rs_wire_coef_kernel(const uint8_t *__restrict__ g, int n, int k, int qtot, uint8_t *__restrict__ coef)
{
    const int total = k * qtot, R = n - k;
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < total; i += (int)(gridDim.x * blockDim.x)) {
        const int t = i / qtot, q = i - t * qtot;
        coef[i] = q < R ? g[(size_t)t * n + k + q] : (uint8_t)0;
    }
}

struct RswArgs {
    int n, k, S, nslices, qtot;
    int64_t nblocks;
    const uint8_t *coef;    // [k][qtot]
    const uint32_t *mul3;   // [256][8]
    const uint8_t *src;     // [nblocks][k][S], 4-byte aligned rows
    const RswDesc *desc;    // [nblocks]
    uint8_t *packets;       // 8-byte aligned, packets of 8 + S bytes: payloads on 4-byte boundaries
};

// Q accumulators per pass (a multiple of 4).  R <= 64 is one pass with Q = R rounded up; a larger R takes further passes over the block's
// slice of the source, 64 parity rows each; only the first pass stores the source packets.
// Slices: ceil(S / 256) of them, slice sl at min(sl * 256, S - 256) -- the last one is moved back to end with the row, the bytes two
// slices share are written twice with the same values -- and a row shorter than a slice leaves the lanes past its end idle.
template <int Q>
__global__ __launch_bounds__(64 * kWaves) void rs_encode_packets_kernel(RswArgs a)
{
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int k = a.k, R = a.n - a.k, S = a.S;
    const uint32_t plen = (uint32_t)S + kHdr;
    cu32 *mul3 = as_const(a.mul3);
    const int64_t nitems = a.nblocks * a.nslices;
    for (int64_t item = (int64_t)blockIdx.x * kWaves + wave; item < nitems; item += (int64_t)gridDim.x * kWaves) {
        const int64_t blk = item / a.nslices;
        const int sl = (int)(item - blk * a.nslices);
        const uint32_t off = (S >= kSlice ? min((uint32_t)sl * kSlice, (uint32_t)(S - kSlice)) : 0u) + (uint32_t)lane * 4u;
        const bool active = off < (uint32_t)S;          // S is a multiple of 4: a dword lies inside the row or outside
        const bool hdr_lane = sl == 0 && lane == 0;     // slice 0 also stores the rows' headers
        cu32 *dw = as_const(a.desc + blk);
        const uint64_t first = (uint64_t)dw[0] | (uint64_t)dw[1] << 32;
        const uint64_t step = (uint64_t)dw[2] * plen;   // bytes between the packets of consecutive rows
        const uint32_t hdr = dw[3];
        uint8_t *pk = a.packets + first * plen;         // the packet of row 0
        const uint8_t *srow = a.src + (uint64_t)blk * (uint64_t)k * (uint64_t)S + off;
        auto store_row = [&](int j, uint32_t v) {
            uint8_t *p = pk + (uint64_t)j * step;
            if (active) __builtin_nontemporal_store(v, reinterpret_cast<uint32_t *>(p + kHdr + off));
            if (hdr_lane) {   // {class, block, symbol} twice (fec_header_dev.h); a packet of 8 + S bytes starts on a 4-byte boundary only
                const uint32_t h = (uint32_t)fec_header(hdr >> 8, hdr, (unsigned)j);
                reinterpret_cast<uint32_t *>(p)[0] = h;
                reinterpret_cast<uint32_t *>(p)[1] = h;
            }
        };
        for (int q0 = 0; q0 < R; q0 += Q) {
            uint32_t acc[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) acc[q] = 0u;
            cu32 *crow = as_const(a.coef + q0);         // row t: crow + t * qtot / 4
            const uint32_t cstep = (uint32_t)a.qtot >> 2;
            uint32_t vcur = active ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(srow)) : 0u;
            for (int t = 0; t < k; t++) {
                // (clamped: the row past the end is the last one again -- an unconditional load keeps the loop branch-free)
                const int tn = t + 1 < k ? t + 1 : t;
                const uint32_t vnxt = active ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(srow + (uint64_t)tn * (uint32_t)S)) : 0u;
                uint32_t cw[Q / 4];
#pragma unroll
                for (int j = 0; j < Q / 4; j++) cw[j] = crow[(uint32_t)t * cstep + j];
                if (q0 == 0) store_row(t, vcur);
                const Sel3 sel = gfsel(vcur);
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    const uint32_t c = (cw[q >> 2] >> (8 * (q & 3))) & 0xffu;
                    acc[q] = gfmac4_sel(acc[q], load_multab(mul3, c), sel);
                }
                vcur = vnxt;
            }
#pragma unroll
            for (int q = 0; q < Q; q++)
                if (q0 + q < R) store_row(k + q0 + q, acc[q]);
        }
    }
}

template <int Q>
void launch_q(ldpc_amd_ctx *ctx, unsigned grid, const RswArgs &a)
{
    hipLaunchKernelGGL(rs_encode_packets_kernel<Q>, dim3(grid), dim3(64 * kWaves), 0, ctx->stream, a);
}

}  // namespace

namespace ldpc_amd {

int launch_rs_encode_packets(ldpc_amd_ctx *ctx, const HostRs &rs, int S, int64_t nblocks, const uint8_t *src, const void *desc, int64_t max_stride,
                             uint8_t *packets)
{
    if (nblocks <= 0) return LDPC_AMD_OK;
    const int R = rs.n - rs.k;
    if (ctx->knobs.enc_pkt == 0 || S < 16 || (S & 3) != 0 || !symbol_len_ok(ctx, S) || R < 1) return kEncodeNotFused;
    // (word form: the source rows are 4-byte aligned whatever the array's alignment, and a packet of 8 + S bytes only every other one)
    if (((uintptr_t)packets & 7) != 0 || ((uintptr_t)src & (symbol_len_words(S) ? 3 : 15)) != 0) return kEncodeNotFused;
    if (!desc || ((uintptr_t)desc & 15) != 0 || max_stride < 1 || (uint64_t)max_stride * (uint64_t)(S + kHdr) >= (1ull << 32)) return kEncodeNotFused;
    const int q = std::min(kQMax, R <= 32 ? (R + 3) & ~3 : (R + 7) & ~7);   // instantiated: 4, 8, ... 32, 40, 48, 56, 64
    const int qtot = (R + q - 1) / q * q;
    int rc;
    if (!ctx->rsw_tab.p) {   // the packed-multiply table, once per context
        static const std::array<uint32_t, 256 * 8> tab = [] {   // built once for the process, never freed: the copy may read it later
            std::array<uint32_t, 256 * 8> t{};
            build_mul3_tables(t.data());
            return t;
        }();
        if ((rc = scratch_reserve(ctx, ctx->rsw_tab, sizeof(tab)))) return rc;
        if (hipMemcpyAsync(ctx->rsw_tab.p, tab.data(), sizeof(tab), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(ctx->rsw_tab.p);
            ctx->rsw_tab = Scratch{};
            return set_error(ctx, LDPC_AMD_EHIP, "rs_encode_packets: the multiply table could not be uploaded");
        }
    }
    if ((rc = scratch_reserve(ctx, ctx->rsw_coef, (size_t)rs.k * qtot))) return rc;
    hipLaunchKernelGGL(rs_wire_coef_kernel, dim3((unsigned)std::min(64, (rs.k * qtot + 255) / 256)), dim3(256), 0, ctx->stream, (const uint8_t *)rs.d_g,
                       rs.n, rs.k, qtot, (uint8_t *)ctx->rsw_coef.p);
    LDPC_HIP_TRY(ctx, hipGetLastError());
    RswArgs a{};
    a.n = rs.n; a.k = rs.k; a.S = S; a.nslices = (S + kSlice - 1) / kSlice; a.qtot = qtot; a.nblocks = nblocks;
    a.coef = (const uint8_t *)ctx->rsw_coef.p; a.mul3 = (const uint32_t *)ctx->rsw_tab.p; a.src = src; a.desc = (const RswDesc *)desc; a.packets = packets;
    // persistent: at most five workgroups (twenty wavefronts) per CU, striding over the (block, slice) items
    const int64_t items = nblocks * a.nslices;
    const unsigned grid = (unsigned)std::min<int64_t>((items + kWaves - 1) / kWaves, (int64_t)ctx->sm_count * 5);
    switch (q) {
        case 4: launch_q<4>(ctx, grid, a); break;
        case 8: launch_q<8>(ctx, grid, a); break;
        case 12: launch_q<12>(ctx, grid, a); break;
        case 16: launch_q<16>(ctx, grid, a); break;
        case 20: launch_q<20>(ctx, grid, a); break;
        case 24: launch_q<24>(ctx, grid, a); break;
        case 28: launch_q<28>(ctx, grid, a); break;
        case 32: launch_q<32>(ctx, grid, a); break;
        case 40: launch_q<40>(ctx, grid, a); break;
        case 48: launch_q<48>(ctx, grid, a); break;
        case 56: launch_q<56>(ctx, grid, a); break;
        default: launch_q<64>(ctx, grid, a); break;
    }
    LDPC_HIP_TRY(ctx, hipGetLastError());
    return LDPC_AMD_OK;
}

}  // namespace ldpc_amd
