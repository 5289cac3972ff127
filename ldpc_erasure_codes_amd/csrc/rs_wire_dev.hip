// rs_wire_dev.hip -- the Reed-Solomon sender of the FEC wire (include/ldpc_erasure_amd_rs_wire.h): source blocks -> wire packets in one
// kernel, every block placed and numbered by the 16-byte descriptor the descriptor-driven senders of wire_dev.hip use.  Behind it the
// decoder of the other end (include/ldpc_erasure_amd_rs_rows.h): the same loop on a per-block table, its rows read where they lie.
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

#include "../../include/ldpc_erasure_amd_rs_rows.h"
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

// ---- the decoder on rows in place (include/ldpc_erasure_amd_rs_rows.h) ---------------------------------------------------------------
// msg = the k source rows of a block, from any k of its n rows.  With the first k usable rows selected (ReedSolomonErasureCodes.m:78-81),
// nsys of them source rows and r = k - nsys repair rows of columns j_0 .. j_{r-1}, and u_0 .. u_{r-1} the missing source positions:
//     msg[u] = sum over the selected rows t of D[t][u] * row_t,
//     D[nsys + q][u] = Minv[u][q],   D[t][u] = sum_q Minv[u][q] * P[pos_t][j_q] for a received source row,   M[q][t] = P[u_t][j_q].
// rs_rows_plan_kernel vets and selects, inverts M on bytes and writes D per block; rs_decode_rows_kernel is then the encoder's loop on
// another table: one wavefront per (block, 256-byte slice), every selected row read once WHERE IT LIES -- the payload of a packet or a
// row of the staging planes, by its source word (internal.h, PacketRows) -- a source row stored to msg, and multiplied into the r
// accumulators.  One pass, no second phase (DESIGN.md 4.4d has the reason and the numbers).
constexpr int kRMax = 64;                       // parity depth n - k the decoder takes
constexpr int kRowsThreads = 256;               // threads of a plan workgroup
constexpr uint8_t kNoLog = 0xFF;                // the plan's logs run 0 .. 254
constexpr size_t kRowsScratchMax = (size_t)256 << 20;

// the accumulators a block runs with follow ITS r, by buckets: 0 (a copy), <= 8, 16, 24, 32, 48, 64
__host__ __device__ constexpr int rows_bucket(int r) { return r <= 8 ? 8 : r <= 16 ? 16 : r <= 24 ? 24 : r <= 32 ? 32 : r <= 48 ? 48 : 64; }

// Per block of a chunk: hdr[4] = {nsys, r, usable rows, status}; rec[k + R][2] = {source word, position} of the k selected rows, then
// {0, position} of the r missing source rows; tab[k][dstride] = D, rows padded with zeros to dstride = rows_bucket(R) bytes.
struct RowsPlanArgs {
    int n, k, dstride;
    int64_t nblocks;
    const uint32_t *src;    // [nblocks][n] source words
    int64_t npackets, nstage_rows;
    const uint8_t *g;       // [k][n] the generator
    uint32_t *hdr, *rec;
    uint8_t *tab;
    uint8_t *er_out;        // [nblocks][n] or nullptr
    int32_t *received, *status;   // [nblocks] or nullptr
};

__global__ __launch_bounds__(kRowsThreads) void rs_rows_plan_kernel(RowsPlanArgs a)
{
    __shared__ uint8_t lg[256], ex[512], pres[256], fcol[kRMax];
    __shared__ uint8_t A[kRMax * 2 * kRMax];    // [r][2 r]: [M | I] -> [I | M^-1]
    __shared__ uint8_t GL[(255 - kRMax) * kRMax];   // [nsys][r], nsys + r = k <= 255, r <= kRMax
    __shared__ uint16_t selpos[256], upos[kRMax];
    __shared__ uint32_t selword[256];
    __shared__ int misc[4];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int n = a.n, k = a.k, R = n - k;
    if (tid == 0) {   // log / antilog of GF(256), polynomial kPrimPoly
        int x = 1;
        for (int i = 0; i < 255; i++) {
            ex[i] = ex[i + 255] = (uint8_t)x;
            lg[x] = (uint8_t)i;
            x <<= 1;
            if (x & 0x100) x ^= kPrimPoly;
        }
        ex[510] = ex[0]; ex[511] = ex[1]; lg[0] = 0;
    }
    auto mul = [&](uint8_t x, uint8_t y) -> uint8_t { return (x && y) ? ex[lg[x] + lg[y]] : (uint8_t)0; };
    const uint64_t below = (1ull << lane) - 1ull;
    for (int64_t blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
        __syncthreads();   // (the tables; the block before is through with the shared arrays)
        pres[tid] = 0;
        if (tid < 64) {    // vet every word, take the first k usable positions in ascending order (rs_select_kernel's rule)
            const uint32_t *w = a.src + blk * n;
            int cnt = 0;
            for (int j0 = 0; j0 < n; j0 += 64) {
                const int j = j0 + lane;
                const uint32_t word = j < n ? w[j] : kRowErased;
                const uint32_t idx = word & ~kRowStaged;
                const bool ok = j < n && word != kRowErased && ((word & kRowStaged) ? (int64_t)idx < a.nstage_rows : (int64_t)idx < a.npackets);
                if (j < n && a.er_out) a.er_out[blk * n + j] = ok ? 0 : 1;
                const uint64_t mask = __ballot(ok);
                const int pos = cnt + __popcll(mask & below);
                if (ok && pos < k) {
                    selpos[pos] = (uint16_t)j;
                    selword[pos] = word;
                }
                cnt += __popcll(mask);
            }
            if (lane == 0) misc[0] = cnt;
        }
        __syncthreads();
        const int cnt = misc[0];
        uint32_t *hdr = a.hdr + blk * 4;
        if (cnt < k) {     // short: no solve, the stream kernel stores zeros
            if (tid == 0) {
                hdr[0] = 0; hdr[1] = 0; hdr[2] = (uint32_t)cnt; hdr[3] = LDPC_AMD_RS_ST_SHORT;
                if (a.received) a.received[blk] = cnt;
                if (a.status) a.status[blk] = LDPC_AMD_RS_ST_SHORT;
            }
            continue;
        }
        for (int t = tid; t < k; t += kRowsThreads)
            if (selpos[t] < k) pres[selpos[t]] = 1;
        __syncthreads();
        if (tid < 64) {    // the missing source positions, ascending
            int miss = 0;
            for (int u0 = 0; u0 < k; u0 += 64) {
                const int u = u0 + lane;
                const bool gone = u < k && pres[u] == 0;
                const uint64_t mask = __ballot(gone);
                const int pos = miss + __popcll(mask & below);
                if (gone && pos < kRMax) upos[pos] = (uint16_t)u;
                miss += __popcll(mask);
            }
            if (lane == 0) { misc[1] = miss; misc[2] = 0; }
        }
        __syncthreads();
        const int r = min(misc[1], min(R, kRMax)), nsys = k - r, W2 = 2 * r;   // (r <= R: the k selected rows hold k - nsys repair rows)
        // selected repair row q is column selpos[nsys + q] of the generator: M[q][t] = g[u_t][that column]
        for (int i = tid; i < r * W2; i += kRowsThreads) {
            const int q = i / W2, c = i - q * W2;
            A[i] = c < r ? a.g[(int)upos[c] * n + selpos[nsys + q]] : (uint8_t)(c - r == q);
        }
        for (int c = 0; c < r; c++) {   // Gauss-Jordan, the first non-zero pivot (rs_decode_kernel)
            __syncthreads();
            if (tid == 0) {
                int p = c;
                while (p < r && A[p * W2 + c] == 0) p++;
                misc[3] = p < r ? p : -1;
            }
            __syncthreads();
            const int p = misc[3];
            if (p < 0) {   // singular: not an MDS generator.  The block is handed out as short.
                if (tid == 0) misc[2] = 1;
                break;
            }
            const uint8_t ipiv = ex[255 - lg[A[p * W2 + c]]];
            __syncthreads();
            if (tid < W2) {   // rows p and c change places, the pivot row scaled to a leading one
                const uint8_t top = A[c * W2 + tid];
                A[c * W2 + tid] = mul(A[p * W2 + tid], ipiv);
                if (p != c) A[p * W2 + tid] = top;
            }
            __syncthreads();
            if (tid < r) fcol[tid] = tid == c ? (uint8_t)0 : A[tid * W2 + c];
            __syncthreads();
            for (int i = tid; i < r * W2; i += kRowsThreads) {
                const int row = i / W2, col = i - row * W2;
                const uint8_t f = fcol[row];
                if (f) A[i] ^= mul(f, A[c * W2 + col]);
            }
        }
        __syncthreads();
        const bool singular = misc[2] != 0;
        if (tid == 0) {
            hdr[0] = singular ? 0u : (uint32_t)nsys; hdr[1] = singular ? 0u : (uint32_t)r; hdr[2] = (uint32_t)cnt;
            hdr[3] = singular ? LDPC_AMD_RS_ST_SHORT : LDPC_AMD_RS_ST_DECODED;
            if (a.received) a.received[blk] = cnt;
            if (a.status) a.status[blk] = singular ? LDPC_AMD_RS_ST_SHORT : LDPC_AMD_RS_ST_DECODED;
        }
        if (singular) continue;
        uint32_t *rec = a.rec + blk * (int64_t)(k + R) * 2;
        for (int t = tid; t < k + r; t += kRowsThreads) {
            rec[2 * t] = t < k ? selword[t] : 0u;
            rec[2 * t + 1] = t < k ? selpos[t] : upos[t - k];
        }
        // D, with every product out of the LDS: the logs of Minv over the left half of A (the identity by now), the logs of the
        // generator entries P[pos_t][j_q] in GL; kNoLog stands for the log of zero
        for (int i = tid; i < r * r; i += kRowsThreads) {
            const int u = i / r, q = i - u * r;
            const uint8_t m = A[u * W2 + r + q];
            A[u * W2 + q] = m ? lg[m] : kNoLog;
        }
        for (int i = tid; i < nsys * r; i += kRowsThreads) {
            const int t = i / r, q = i - t * r;
            const uint8_t c = a.g[(int)selpos[t] * n + selpos[nsys + q]];
            GL[i] = c ? lg[c] : kNoLog;
        }
        __syncthreads();
        uint8_t *tab = a.tab + blk * (int64_t)k * a.dstride;
        for (int i = tid; i < nsys * r; i += kRowsThreads) {       // a received source row: D[t][u] = sum_q Minv[u][q] P[pos_t][j_q]
            const int t = i / r, u = i - t * r;
            const uint8_t *ml = A + u * W2, *gl = GL + t * r;
            uint8_t d = 0;
            for (int q = 0; q < r; q++) {
                const uint8_t x = ml[q], y = gl[q];
                if (x != kNoLog && y != kNoLog) d ^= ex[x + y];
            }
            tab[t * a.dstride + u] = d;
        }
        for (int i = tid; i < r * r; i += kRowsThreads) {          // a selected repair row: D[nsys + q][u] = Minv[u][q]
            const int q = i / r, u = i - q * r;
            tab[(nsys + q) * a.dstride + u] = A[u * W2 + r + q];
        }
        const int pad = a.dstride - r;                              // the columns past r: zero coefficients
        for (int i = tid; i < k * pad; i += kRowsThreads) {
            const int t = i / pad, u = r + (i - t * pad);
            tab[t * a.dstride + u] = 0;
        }
    }
}

struct RowsArgs {
    int k, nrec, S, nslices, dstride;   // nrec = k + R records per block
    int64_t nblocks;
    const uint32_t *mul3;   // [256][8]
    const uint32_t *hdr, *rec;
    const uint8_t *tab;
    const uint8_t *packets, *stage;   // packets of 8 + S bytes, 8-byte aligned; rows of S bytes, 4-byte aligned
    uint8_t *msg;                     // [nblocks][k][S], 4-byte aligned
};

// One decoded block's slice with Q >= r accumulators (Q = 0: every source row arrived, a copy).  Row t + 1 is in flight while row t is
// multiplied, and the record of row t + 2 -- where it lies -- is on its way from the scalar cache.
template <int Q>
__device__ __forceinline__ void rows_block(const RowsArgs &a, cu32 *rec, cu32 *tab, cu32 *mul3, uint8_t *mrow, int nsys, int r, bool active, uint32_t off)
{
    const int k = a.k;
    const uint32_t S = (uint32_t)a.S, plen = S + kHdr;
    auto row = [&](uint32_t w) {   // w wave-uniform and vetted by the plan: inside its array
        const uint8_t *p = (w & kRowStaged) ? a.stage + (uint64_t)(w & ~kRowStaged) * S : a.packets + (uint64_t)w * plen + kHdr;
        return reinterpret_cast<const uint32_t *>(p + off);
    };
    uint32_t acc[Q > 0 ? Q : 1];
#pragma unroll
    for (int q = 0; q < Q; q++) acc[q] = 0u;
    const uint32_t cstep = (uint32_t)a.dstride >> 2;
    const int t1 = k > 1 ? 1 : 0;
    uint32_t vcur = active ? __builtin_nontemporal_load(row(rec[0])) : 0u;
    uint32_t pcur = rec[1], wnxt = rec[2 * t1], pnxt = rec[2 * t1 + 1];
    for (int t = 0; t < k; t++) {
        // (clamped: the row past the end is the last one again, as in the encoder)
        const uint32_t vnxt = active ? __builtin_nontemporal_load(row(wnxt)) : 0u;
        const int t2 = t + 2 < k ? t + 2 : k - 1;
        const uint32_t w2 = rec[2 * t2], p2 = rec[2 * t2 + 1];
        if (t < nsys && active) __builtin_nontemporal_store(vcur, reinterpret_cast<uint32_t *>(mrow + (uint64_t)pcur * S));
        if constexpr (Q > 0) {
            uint32_t cw[Q / 4];
#pragma unroll
            for (int j = 0; j < Q / 4; j++) cw[j] = tab[(uint32_t)t * cstep + j];
            const Sel3 sel = gfsel(vcur);
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const uint32_t c = (cw[q >> 2] >> (8 * (q & 3))) & 0xffu;
                acc[q] = gfmac4_sel(acc[q], load_multab(mul3, c), sel);
            }
        }
        vcur = vnxt; pcur = pnxt; wnxt = w2; pnxt = p2;
    }
#pragma unroll
    for (int q = 0; q < Q; q++)
        if (q < r && active) __builtin_nontemporal_store(acc[q], reinterpret_cast<uint32_t *>(mrow + (uint64_t)rec[2 * (k + q) + 1] * S));
}

__global__ __launch_bounds__(64 * kWaves) void rs_decode_rows_kernel(RowsArgs a)
{
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int k = a.k, S = a.S;
    cu32 *mul3 = as_const(a.mul3);
    const int64_t nitems = a.nblocks * a.nslices;
    for (int64_t item = (int64_t)blockIdx.x * kWaves + wave; item < nitems; item += (int64_t)gridDim.x * kWaves) {
        const int64_t blk = item / a.nslices;
        const int sl = (int)(item - blk * a.nslices);
        const uint32_t off = (S >= kSlice ? min((uint32_t)sl * kSlice, (uint32_t)(S - kSlice)) : 0u) + (uint32_t)lane * 4u;
        const bool active = off < (uint32_t)S;
        cu32 *hdr = as_const(a.hdr + blk * 4);
        const int nsys = (int)hdr[0], r = (int)hdr[1];
        uint8_t *mrow = a.msg + (uint64_t)blk * (uint64_t)k * (uint64_t)S + off;
        if (hdr[3] != (uint32_t)LDPC_AMD_RS_ST_DECODED) {   // short: zeros over all k rows
            for (int t = 0; t < k; t++)
                if (active) __builtin_nontemporal_store(0u, reinterpret_cast<uint32_t *>(mrow + (uint64_t)t * (uint32_t)S));
            continue;
        }
        cu32 *rec = as_const(a.rec + blk * a.nrec * 2);
        cu32 *tab = as_const(a.tab + blk * (int64_t)k * a.dstride);
        // wave-uniform: r came through a scalar load
        if (r == 0) rows_block<0>(a, rec, tab, mul3, mrow, nsys, r, active, off);
        else if (r <= 8) rows_block<8>(a, rec, tab, mul3, mrow, nsys, r, active, off);
        else if (r <= 16) rows_block<16>(a, rec, tab, mul3, mrow, nsys, r, active, off);
        else if (r <= 24) rows_block<24>(a, rec, tab, mul3, mrow, nsys, r, active, off);
        else if (r <= 32) rows_block<32>(a, rec, tab, mul3, mrow, nsys, r, active, off);
        else if (r <= 48) rows_block<48>(a, rec, tab, mul3, mrow, nsys, r, active, off);
        else rows_block<64>(a, rec, tab, mul3, mrow, nsys, r, active, off);
    }
}

// the packed-multiply table of the context, uploaded once
int rsw_table(ldpc_amd_ctx *ctx, const char *who)
{
    if (ctx->rsw_tab.p) return LDPC_AMD_OK;
    static const std::array<uint32_t, 256 * 8> tab = [] {   // built once for the process, never freed: the copy may read it later
        std::array<uint32_t, 256 * 8> t{};
        build_mul3_tables(t.data());
        return t;
    }();
    int rc;
    if ((rc = scratch_reserve(ctx, ctx->rsw_tab, sizeof(tab)))) return rc;
    if (hipMemcpyAsync(ctx->rsw_tab.p, tab.data(), sizeof(tab), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(ctx->rsw_tab.p);
        ctx->rsw_tab = Scratch{};
        return set_error(ctx, LDPC_AMD_EHIP, "%s: the multiply table could not be uploaded", who);
    }
    return LDPC_AMD_OK;
}

// bytes of plan scratch per block, and where the three arrays of a chunk of `count` blocks begin
struct RowsLayout {
    size_t per_block, o_rec, o_tab, bytes;
    int dstride;
    int64_t chunk;
};
RowsLayout rows_layout(const HostRs &rs, int64_t nblocks)
{
    const int R = rs.n - rs.k;
    RowsLayout l{};
    l.dstride = rows_bucket(R);
    l.per_block = 16 + (size_t)rs.n * 8 + (size_t)rs.k * l.dstride;
    l.chunk = std::max<int64_t>(1, std::min<int64_t>(nblocks, (int64_t)((kRowsScratchMax - 512) / l.per_block)));
    l.o_rec = ((size_t)l.chunk * 16 + 255) & ~(size_t)255;
    l.o_tab = (l.o_rec + (size_t)l.chunk * rs.n * 8 + 255) & ~(size_t)255;
    l.bytes = l.o_tab + (size_t)l.chunk * rs.k * l.dstride;
    return l;
}

}  // namespace

namespace ldpc_amd {

bool rs_decode_rows_takes(const ldpc_amd_ctx *ctx, const HostRs &rs, int S, const uint8_t *packets, const uint8_t *stage, const uint8_t *msg)
{
    const int R = rs.n - rs.k;
    if (ctx->knobs.rx_pkt == 0 || R < 1 || R > kRMax || rs.n > 256) return false;
    if (S < 16 || (S & 3) != 0 || !symbol_len_ok(ctx, S)) return false;   // every access is a dword one: the word form needs nothing extra
    // (row addresses are 64-bit products of a word below 2^31 and 8 + S or S: any array the words can name is addressable)
    return ((uintptr_t)packets & 7) == 0 && ((uintptr_t)stage & 3) == 0 && ((uintptr_t)msg & 3) == 0;
}

bool rs_decode_rows_fused(const ldpc_amd_ctx *ctx, const HostRs &rs, int S, const uint8_t *packets, const uint8_t *stage, const uint8_t *msg)
{
    // Where launch_rs_decode_frames streams already (rs_decode_packets_kernel: R <= 32, S a multiple of 256 or a word length from 256
    // up) the fused form would save only the gather, and loses more than that: RS(255,223), S = 1024, 4096 blocks at 10 % loss, rows
    // in place 2.27 ms against 1.38 + 0.60 ms of gather (profiles/rs_rows_bench.json).  Those shapes stay composed.
    const int R = rs.n - rs.k;
    if (R <= 32 && rs.k <= 256 && S >= 256 && ((S % 256) == 0 || symbol_len_words(S)) && S < (1 << 23) && ctx->knobs.rs_generic == 0) return false;
    return rs_decode_rows_takes(ctx, rs, S, packets, stage, msg);
}

int rs_decode_rows_reserve(ldpc_amd_ctx *ctx, const HostRs &rs, int64_t nblocks, size_t *bytes)
{
    *bytes = 0;
    if (nblocks <= 0) return LDPC_AMD_OK;
    int rc;
    if ((rc = rsw_table(ctx, "rs_decode_rows"))) return rc;
    return scratch_reserve(ctx, ctx->rsr_plan, *bytes = rows_layout(rs, nblocks).bytes);
}

int launch_rs_decode_rows(ldpc_amd_ctx *ctx, const HostRs &rs, int S, int64_t nblocks, const PacketRows &rows, int64_t npackets,
                          int64_t nstage_rows, uint8_t *er_out, uint8_t *msg, int32_t *received, int32_t *status, int *launches)
{
    if (launches) *launches = 0;
    if (nblocks <= 0) return LDPC_AMD_OK;
    if (!rs_decode_rows_takes(ctx, rs, S, rows.packets, rows.stage, msg) || ((uintptr_t)rows.src & 3) != 0) return kDecodeNotFused;
    int rc;
    size_t bytes;
    if ((rc = rs_decode_rows_reserve(ctx, rs, nblocks, &bytes))) return rc;
    const RowsLayout l = rows_layout(rs, nblocks);
    uint8_t *ws = (uint8_t *)ctx->rsr_plan.p;
    const int n = rs.n, k = rs.k;
    for (int64_t first = 0; first < nblocks; first += l.chunk) {   // the chunks follow one another on the stream: one scratch
        const int64_t count = std::min(l.chunk, nblocks - first);
        RowsPlanArgs p{};
        p.n = n; p.k = k; p.dstride = l.dstride; p.nblocks = count; p.src = rows.src + first * n; p.npackets = npackets; p.nstage_rows = nstage_rows;
        p.g = rs.d_g; p.hdr = (uint32_t *)ws; p.rec = (uint32_t *)(ws + l.o_rec); p.tab = ws + l.o_tab;
        p.er_out = er_out ? er_out + first * n : nullptr; p.received = received ? received + first : nullptr; p.status = status ? status + first : nullptr;
        hipLaunchKernelGGL(rs_rows_plan_kernel, dim3((unsigned)std::min<int64_t>(count, (int64_t)ctx->sm_count * 8)), dim3(kRowsThreads), 0, ctx->stream, p);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        RowsArgs a{};
        a.k = k; a.nrec = n; a.S = S; a.nslices = (S + kSlice - 1) / kSlice; a.dstride = l.dstride; a.nblocks = count;
        a.mul3 = (const uint32_t *)ctx->rsw_tab.p; a.hdr = p.hdr; a.rec = p.rec; a.tab = p.tab; a.packets = rows.packets; a.stage = rows.stage;
        a.msg = msg + (size_t)first * k * S;
        // persistent, the encoder's grid: at most five workgroups (twenty wavefronts) per CU, striding over the (block, slice) items
        const int64_t items = count * a.nslices;
        const unsigned grid = (unsigned)std::min<int64_t>((items + kWaves - 1) / kWaves, (int64_t)ctx->sm_count * 5);
        hipLaunchKernelGGL(rs_decode_rows_kernel, dim3(grid), dim3(64 * kWaves), 0, ctx->stream, a);
        LDPC_HIP_TRY(ctx, hipGetLastError());
        if (launches) ++*launches;
    }
    return LDPC_AMD_OK;
}

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
    if ((rc = rsw_table(ctx, "rs_encode_packets"))) return rc;
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

// ---- the decoder alone (include/ldpc_erasure_amd_rs_rows.h): everything is checked before anything is enqueued ---------------------------
extern "C" int ldpc_amd_rs_decode_rows_dev(ldpc_amd_ctx *ctx, int rs, int S, int64_t nblocks, const uint32_t *src, const uint8_t *packets,
                                           int64_t npackets, const uint8_t *stage, int64_t nstage_rows, uint8_t *msg, int32_t *received,
                                           int32_t *status, uint8_t *erased_out)
{
    if (!ctx) return LDPC_AMD_EINVAL;
    if (rs < 0 || rs >= (int)ctx->rs.size()) return set_error(ctx, LDPC_AMD_ENOCODE, "unknown RS handle %d", rs);
    const HostRs &r = *ctx->rs[rs];
    if (nblocks < 0 || npackets < 0 || nstage_rows < 0 || S < 1)
        return set_error(ctx, LDPC_AMD_EINVAL, "rs_decode_rows: need nblocks, npackets, nstage_rows >= 0 and S >= 1");
    if (nblocks * r.n >= ((int64_t)1 << 31) || nblocks >= ((int64_t)1 << 31))
        return set_error(ctx, LDPC_AMD_EINVAL, "rs_decode_rows: nblocks * n must be below 2^31");
    if (npackets >= ((int64_t)1 << 31) || nstage_rows >= ((int64_t)1 << 31))
        return set_error(ctx, LDPC_AMD_EINVAL, "rs_decode_rows: a source word names packets and staged rows below 2^31");
    if (nblocks == 0) return LDPC_AMD_OK;
    if (npackets == 0) packets = nullptr;
    if (nstage_rows == 0) stage = nullptr;
    if (S == 1 || r.n - r.k > kRMax) return set_error(ctx, LDPC_AMD_EUNSUP, "rs_decode_rows: S = 1 and n - k > %d have no decoder on rows in place", kRMax);
    if (!symbol_len_ok(ctx, S)) return refuse_symbol_len(ctx, S, "S must be a multiple of 16 (got %d)");
    LDPC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const void *need[] = {src, msg, npackets ? packets : msg, nstage_rows ? stage : msg};
    const void *opt[] = {received, status, erased_out};
    bool ok = true;
    for (const void *p : need) ok = ok && p && is_device_ptr(ctx, p);
    for (const void *p : opt) ok = ok && (!p || is_device_ptr(ctx, p));
    if (!ok) return set_error(ctx, LDPC_AMD_EINVAL, "rs_decode_rows: src, packets, stage, msg and the result arrays must be device pointers of device %d", ctx->device);
    const uintptr_t m0 = (uintptr_t)msg, m1 = m0 + (size_t)nblocks * r.k * S;
    auto overlaps = [&](const void *p, size_t bytes) { return p && (uintptr_t)p < m1 && m0 < (uintptr_t)p + bytes; };
    if (overlaps(packets, (size_t)npackets * (S + kHdr)) || overlaps(stage, (size_t)nstage_rows * S) || overlaps(src, (size_t)nblocks * r.n * 4))
        return set_error(ctx, LDPC_AMD_EINVAL, "rs_decode_rows: msg must not overlap packets, stage or src");
    if (!rs_decode_rows_takes(ctx, r, S, packets, stage, msg) || ((uintptr_t)src & 3) != 0)
        return set_error(ctx, LDPC_AMD_EUNSUP, "rs_decode_rows: needs packets 8-byte aligned, stage, msg and src 4-byte aligned, and the knob RX_PKT not 0");
    const int rc = launch_rs_decode_rows(ctx, r, S, nblocks, PacketRows{src, packets, stage, S + kHdr}, npackets, nstage_rows, erased_out, msg, received, status);
    return rc == kDecodeNotFused ? set_error(ctx, LDPC_AMD_EUNSUP, "rs_decode_rows: no decoder on rows in place for this call") : rc;
}
