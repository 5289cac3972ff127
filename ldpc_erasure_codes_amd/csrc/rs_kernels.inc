// rs_kernels.inc -- Reed-Solomon erasure decode / encode (included by kernels.hip inside its anonymous
// namespace).  Reference: Matlab/My_RS_Decode_Optimize_With_GFTables.m:15-118 (decode),
// Matlab/Test_My_RS_Decode.m:30-37,48 (generator, encode).
//
// The reference builds the k x k matrix of the received columns of the systematic generator, moves the
// received systematic symbols to an identity block by column swaps (:29-48), eliminates the repair rows
// against it (:55-91) and back-substitutes (:100-105).  Because G = [I | P] is MDS, every k received
// columns are independent and the solution is unique; what the elimination really solves is the r x r
// system of the r = k - N_sys missing source symbols against the r received repair symbols:
//
//      sum_{u missing} s_u P[u][j_q] = c_{j_q} + sum_{i received} s_i P[i][j_q]        q = 0..r-1
//
// The kernel solves exactly that system (first-non-zero pivoting like :70-90), which gives the same bytes
// as the reference on every input it can decode.  M^-1 depends only on the erasure pattern and is shared
// by the S byte lanes of a packet.
struct RsArgs {
    int n, k, S;
    int64_t nblocks;
    const uint8_t *pt;        // [n-k][k]   P transposed
    const uint16_t *recv_idx; // [nblocks][k]
    const uint8_t *recv_val;  // [nblocks][k][S]; FRAMES: the frames [nblocks][n][S], row t of a block is read in place at recv_idx[t] * S
    const int32_t *nrecv;     // FRAMES: [nblocks] symbols received; a block with fewer than k decodes to zeros (ReedSolomonErasureCodes.m:78,80)
    uint8_t *msg;             // [nblocks][k][S]
    uint8_t *ws;              // [gridDim.x][n-k][S]  (packets only)
    int *bad;                 // device counter: blocks with malformed positions (decoded to zeros), or nullptr
    int lds_idx, lds_pres, lds_ulist, lds_M, lds_b, lds_lg, lds_ex, lds_misc;
};

// FRAMES (all three decode kernels): the input is the frame format (sym [nblocks][n][S] + the positions rs_select_kernel took from
// the erasure flags) instead of gathered rows.  A compile-time switch: the instantiations of ldpc_amd_rs_decode_batch keep their code.
//
// The selection: P = the ascending positions with erased == 0; the first k of them are what the reference's loop step hands to the
// decoder (ReedSolomonErasureCodes.m:80-81), |P| is reported, fewer than k is a block that cannot be decoded (:78).  One wavefront
// per block: a ballot over 64 flags, a lane's place in P is the count of the received lanes below it (mbcnt) plus the rounds before.
__global__ __launch_bounds__(256) void rs_select_kernel(int n, int k, int64_t nblocks, const uint8_t *erased, uint16_t *idx /* [nblocks][k] */,
                                                        int32_t *nrecv, int32_t *received, int32_t *status)
{
    const int lane = lane_id(), nw = (int)(blockDim.x >> 6);
    const int64_t blk = (int64_t)blockIdx.x * nw + wave_id();
    if (blk >= nblocks) return;
    const uint8_t *er = erased + blk * n;
    uint16_t *ix = idx + blk * k;
    const uint64_t lt = (1ull << lane) - 1ull;
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += kWave) {
        const int j = j0 + lane;
        const bool rec = j < n && er[j] == 0;
        const uint64_t mask = __ballot(rec);
        const int pos = cnt + __popcll(mask & lt);
        if (rec && pos < k) ix[pos] = (uint16_t)j;
        cnt += __popcll(mask);
    }
    if (lane == 0) {
        nrecv[blk] = cnt;
        if (received) received[blk] = cnt;
        if (status) status[blk] = cnt < k ? LDPC_AMD_RS_ST_SHORT : LDPC_AMD_RS_ST_DECODED;
    }
}

// 16 bytes of a row; w4 (wave-uniform): the row is only 4-byte aligned (S a multiple of 4, not of 16) -- four dword accesses
__device__ __forceinline__ U4 rs_ld16(const uint8_t *p, bool w4) { return w4 ? row_load16<true>(p) : row_load16<false>(p); }
__device__ __forceinline__ void rs_st16(uint8_t *p, const U4 &v, bool w4)
{
    if (w4) row_store16<true>(p, v);
    else row_store16<false>(p, v);
}

template <bool FRAMES>
__global__ __launch_bounds__(256) void rs_decode_kernel(RsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int k = a.k, R = a.n - a.k, S = a.S;
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int lane = lane_id(), wave = wave_id(), nw = nthr >> 6;
    uint16_t *sidx = reinterpret_cast<uint16_t *>(smem + a.lds_idx);
    uint8_t *pres = smem + a.lds_pres;
    uint8_t *ulist = smem + a.lds_ulist;
    uint8_t *M = smem + a.lds_M;       // [R][2R]
    uint8_t *bvec = smem + a.lds_b;    // [R]
    uint8_t *lg = smem + a.lds_lg, *ex = smem + a.lds_ex;
    int *misc = reinterpret_cast<int *>(smem + a.lds_misc);
    const int W2 = 2 * R;

    for (int i = tid; i < 256; i += nthr) lg[i] = c_log[i];
    for (int i = tid; i < 512; i += nthr) ex[i] = c_exp[i];

    for (int64_t blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
        const uint16_t *idx = a.recv_idx + blk * k;
        const uint8_t *val = a.recv_val + blk * (int64_t)(FRAMES ? a.n : k) * S;
        uint8_t *out = a.msg + blk * (int64_t)k * S;
        auto rw = [&](int t) { return FRAMES ? (size_t)sidx[t] : (size_t)t; };   // row of val that holds received symbol t
        __syncthreads();
        if (FRAMES && a.nrecv[blk] < k) {   // short block (workgroup-uniform): zeros, no solve
            for (int64_t i = tid; i < (int64_t)k * S; i += nthr) out[i] = 0;
            continue;
        }
        if (tid == 0) { misc[0] = 0; misc[1] = 0; }
        for (int i = tid; i < k; i += nthr) pres[i] = 0;
        __syncthreads();
        {   // num_sys_symbols = length(find(recv_vec_ind <= k))   (:29)
            int c = 0;
            bool bad = false;
            for (int t = tid; t < k; t += nthr) {
                const uint16_t v = idx[t];
                sidx[t] = v;
                // precondition of the reference's caller (ReedSolomonErasureCodes.m:80-81): positions < n, strictly ascending
                bad = bad || v >= a.n || (t > 0 && idx[t - 1] >= v);
                if (v < k) { c++; pres[v] = 1; }
            }
            if (c) atomicAdd(&misc[0], c);
            if (bad) misc[1] = 1;
        }
        __syncthreads();
        if (misc[1]) {   // malformed block (workgroup-uniform): no table is indexed with it, the block decodes to zeros
            for (int64_t i = tid; i < (int64_t)k * S; i += nthr) out[i] = 0;
            if (tid == 0 && a.bad) atomicAdd(a.bad, 1);
            continue;
        }
        const int nsys = misc[0];
        const int r = k - nsys;
        if (wave == 0) {   // the missing source positions, ascending
            int cnt = 0;
            for (int i0 = 0; i0 < k; i0 += kWave) {
                const int i = i0 + lane;
                const bool miss = (i < k) && !pres[i];
                const uint64_t mask = __ballot(miss);
                if (miss) ulist[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = (uint8_t)i;
                cnt += __popcll(mask);
            }
        }
        __syncthreads();
        // [M | I] : M[q][t] = P[ulist[t]][j_q],  j_q = idx[nsys+q] - k
        for (int e = tid; e < r * r; e += nthr) {
            const int q = e / r, t = e - q * r;
            const int j = (int)sidx[nsys + q] - k;
            M[q * W2 + t] = a.pt[(size_t)j * k + ulist[t]];
            M[q * W2 + r + t] = (q == t) ? 1 : 0;
        }
        __syncthreads();
        // Gauss-Jordan -> M^-1 in the right half (wave 0; lanes over the 2r columns)
        if (wave == 0) {
            for (int col = 0; col < r; col++) {
                int p = -1;
                for (int q0 = col; q0 < r && p < 0; q0 += kWave) {
                    const int q = q0 + lane;
                    const uint64_t mask = __ballot(q < r && M[q * W2 + col] != 0);
                    if (mask) p = q0 + __ffsll((long long)mask) - 1;
                }
                if (p < 0) break;  // cannot happen for an MDS generator; leaves zeros
                const uint32_t piv = M[p * W2 + col];
                const uint32_t linv = (255u - lg[piv]) % 255u;
                wave_sync();
                for (int c = lane; c < W2; c += kWave) {
                    const uint32_t vp = M[p * W2 + c], vc = M[col * W2 + c];
                    const uint32_t sc = vp ? ex[lg[vp] + linv] : 0u;
                    if (p != col) M[p * W2 + c] = (uint8_t)vc;
                    M[col * W2 + c] = (uint8_t)sc;
                }
                wave_sync();
                for (int q = 0; q < r; q++) {
                    if (q == col) continue;
                    const uint32_t f = M[q * W2 + col];
                    if (!f) continue;
                    const uint32_t lf = lg[f];
                    wave_sync();
                    for (int c = lane; c < W2; c += kWave) {
                        const uint32_t v = M[col * W2 + c];
                        if (v) M[q * W2 + c] ^= ex[lg[v] + lf];
                    }
                }
                wave_sync();
            }
        }
        __syncthreads();

        if (S == 1) {
            // b_q = c_{j_q} + sum_{t < nsys} P[idx[t]][j_q] * val[t]
            for (int q = wave; q < r; q += nw) {
                const int j = (int)sidx[nsys + q] - k;
                uint32_t acc = 0;
                for (int t = lane; t < nsys; t += kWave) {
                    const uint32_t c = a.pt[(size_t)j * k + sidx[t]], v = val[rw(t)];
                    if (c && v) acc ^= ex[lg[c] + lg[v]];
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) acc ^= __shfl_xor(acc, d);
                if (lane == 0) bvec[q] = (uint8_t)(acc ^ val[rw(nsys + q)]);
            }
            __syncthreads();
            for (int t = tid; t < r; t += nthr) {
                uint32_t x = 0;
                for (int q = 0; q < r; q++) {
                    const uint32_t c = M[t * W2 + r + q], v = bvec[q];
                    if (c && v) x ^= ex[lg[c] + lg[v]];
                }
                out[ulist[t]] = (uint8_t)x;
            }
            for (int t = tid; t < nsys; t += nthr) out[sidx[t]] = val[rw(t)];
        } else {
            uint8_t *ws = a.ws + (size_t)blockIdx.x * R * S;
            // Word form (S a multiple of 4, not of 16; off the hot path, so a run-time switch): ceil(S / 16) chunks, the last one moved
            // back to end with the row, 4-byte accesses (rs_ld16 / rs_st16).  The chunk that overlaps its neighbour is computed by two lanes
            // of one wavefront from the same bytes: the rows of val are only read, the rows of ws and out are each written by ONE
            // wavefront, and ws is read back only behind the barrier.
            const bool w4 = (S & 15) != 0;
            const int chunks = (S + 15) >> 4;
            auto co = [&](int i) { return w4 ? min(i * 16, S - 16) : i * 16; };
            for (int q = wave; q < r; q += nw) {
                const int j = (int)sidx[nsys + q] - k;
                for (int i = lane; i < chunks; i += kWave) {
                    U4 acc = rs_ld16(val + rw(nsys + q) * S + co(i), w4);
                    for (int t = 0; t < nsys; t++) {
                        const uint32_t c = uniform(a.pt[(size_t)j * k + sidx[t]]);
                        const U4 v = rs_ld16(val + rw(t) * S + co(i), w4);
                        gfmac16(acc, load_multab(c), v);
                    }
                    rs_st16(ws + (size_t)q * S + co(i), acc, w4);
                }
            }
            __syncthreads();
            for (int t = wave; t < r; t += nw) {
                for (int i = lane; i < chunks; i += kWave) {
                    U4 acc = {0, 0, 0, 0};
                    for (int q = 0; q < r; q++) {
                        const uint32_t c = uniform(M[t * W2 + r + q]);
                        const U4 v = rs_ld16(ws + (size_t)q * S + co(i), w4);
                        gfmac16(acc, load_multab(c), v);
                    }
                    rs_st16(out + (size_t)ulist[t] * S + co(i), acc, w4);
                }
            }
            for (int t = wave; t < nsys; t += nw)
                for (int i = lane; i < chunks; i += kWave)
                    rs_st16(out + (size_t)sidx[t] * S + co(i), rs_ld16(val + rw(t) * S + co(i), w4), w4);
        }
    }
}

// ---- S = 1, n - k <= 32: one WAVEFRONT per block, the whole r x r system in registers ----------------------------
// Lane q owns row q of [M | b] (M: r <= 32 bytes = 8 dwords).  Per column: ballot for the first non-zero row at or
// below the diagonal (the reference's swap_ind search, :78-90), the pivot row is broadcast with v_readlane, every other
// row with a non-zero in the column subtracts its multiple (multiplier f / pivot, multiply table picked by log from
// LDS).  No scaling pass and no back substitution: Gauss-Jordan leaves a diagonal system, x_q = b_q / d_q.  MDS => the
// solution is unique, so the bytes equal the reference's.  Tables (log P, log, antilog, multiply-by-alpha^l) are staged
// once per workgroup; wavefronts never meet at a barrier inside the block loop.
struct RsFastLds {
    int lgp, lg16, ex, mtl, wave0, wstride;   // per wave: sidx u16[256] | sval u8[256] | pres u8[256] | ulist u8[32]
};

template <bool FRAMES>
__global__ __launch_bounds__(256) void rs_decode_s1_kernel(RsArgs a, RsFastLds L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int k = a.k, R = a.n - a.k;
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int lane = lane_id(), wave = wave_id(), nw = nthr >> 6;
    uint8_t *lgP = smem + L.lgp;                                          // [R][k] log of P transposed
    uint16_t *lg16 = reinterpret_cast<uint16_t *>(smem + L.lg16);        // log, lg16[0] = 511 (=> antilog index >= 510 => 0)
    uint8_t *ex = smem + L.ex;                                            // [1024]: alpha^(i mod 255) for i < 510, else 0
    uint32_t *mtl = reinterpret_cast<uint32_t *>(smem + L.mtl);          // [255][8] multiply tables by log
    unsigned char *wbase = smem + L.wave0 + wave * L.wstride;
    uint16_t *sidx = reinterpret_cast<uint16_t *>(wbase);
    uint8_t *sval = wbase + 512, *pres = wbase + 768, *ulist = wbase + 1024;

    for (int i = tid; i < R * k; i += nthr) lgP[i] = c_log[a.pt[i]];     // entries of an MDS generator are non-zero
    for (int i = tid; i < 256; i += nthr) lg16[i] = i ? (uint16_t)c_log[i] : (uint16_t)511;
    for (int i = tid; i < 1024; i += nthr) ex[i] = i < 510 ? c_exp[i % 255] : (uint8_t)0;
    for (int i = tid; i < 2048; i += nthr) mtl[i] = c_mul3[(uint32_t)c_exp[i >> 3] * 8 + (i & 7)];
    __syncthreads();

    const uint64_t lt = (1ull << lane) - 1ull;
    for (int64_t blk = (int64_t)blockIdx.x * nw + wave; blk < a.nblocks; blk += (int64_t)gridDim.x * nw) {
        const uint16_t *idx = a.recv_idx + blk * k;
        const uint8_t *val = a.recv_val + blk * (FRAMES ? a.n : k);
        uint8_t *out = a.msg + blk * k;
        uint32_t id[4], vv[4], lv[4];
        int nsys = 0;
        wave_sync();
        if constexpr (FRAMES) {
            if (a.nrecv[blk] < k) {   // short block (wave-uniform): zeros, no solve
                for (int t = lane; t < k; t += kWave) out[t] = 0;
                continue;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = u * 64 + lane;
            id[u] = t < k ? (uint32_t)idx[t] : 0xFFFFu;
            if constexpr (FRAMES) vv[u] = t < k ? (uint32_t)val[id[u]] : 0u;   // (id < n: the selection's positions)
            else vv[u] = t < k ? (uint32_t)val[t] : 0u;
            pres[t] = 0;
        }
        {   // positions must be < n and strictly ascending (ReedSolomonErasureCodes.m:80-81); a malformed block decodes to zeros
            bool bad = false;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int t = u * 64 + lane;
                if (t < k) bad = bad || id[u] >= (uint32_t)a.n || (t > 0 && (uint32_t)idx[t - 1] >= id[u]);
            }
            if (__ballot(bad)) {   // wave-uniform
                for (int t = lane; t < k; t += kWave) out[t] = 0;
                if (lane == 0 && a.bad) atomicAdd(a.bad, 1);
                continue;
            }
        }
        wave_sync();
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = u * 64 + lane;
            const bool sys = id[u] < (uint32_t)k;      // num_sys_symbols = length(find(recv_vec_ind <= k))   (:29)
            if (sys) pres[id[u]] = 1;
            sidx[t] = (uint16_t)id[u];
            sval[t] = (uint8_t)vv[u];
            lv[u] = lg16[vv[u]];
            nsys += __popcll(__ballot(sys));
        }
        wave_sync();
        const int r = k - nsys;
        {   // the missing source positions, ascending
            int cnt = 0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = u * 64 + lane;
                const bool miss = (i < k) && !pres[i];
                const uint64_t mask = __ballot(miss);
                if (miss) ulist[cnt + __popcll(mask & lt)] = (uint8_t)i;
                cnt += __popcll(mask);
            }
        }
        wave_sync();
        const bool rowl = lane < r;
        const int jq = rowl ? (int)sidx[nsys + lane] - k : 0;
        const uint8_t *lgPj = lgP + jq * k;
        // b_q = c_{j_q} + sum_{t < nsys} P[idx[t]][j_q] * val[t]   (entries t < nsys are the received source symbols).
        // Lanes run over t (all 64 busy, four entries each), rows q are taken four at a time: the four partial sums
        // sit in the four bytes of one register, so ONE xor-butterfly over the wavefront reduces four rows.
        uint32_t b = rowl ? (uint32_t)sval[nsys + lane] : 0u;
        bool tv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) tv[u] = u * 64 + lane < nsys;
#pragma unroll
        for (int q0 = 0; q0 < 32; q0 += 4) {
            if (q0 < r) {
                uint32_t packed = 0;
#pragma unroll
                for (int z = 0; z < 4; z++) {
                    // rows past r reuse row 0's table: their sums land in lanes >= r, which never read them
                    const int jz = __builtin_amdgcn_readlane(jq, q0 + z);
                    const uint8_t *base = lgP + jz * k;
                    uint32_t e4[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) e4[u] = tv[u] ? (uint32_t)base[id[u]] + lv[u] : 1023u;   // ex[1023] = 0
                    uint32_t part = 0;
#pragma unroll
                    for (int u = 0; u < 4; u++) part ^= ex[e4[u]];
                    packed |= part << (8 * z);
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) packed ^= (uint32_t)__shfl_xor((int)packed, d);
                const int z = lane - q0;
                if (z >= 0 && z < 4) b ^= (packed >> (8 * z)) & 0xFFu;
            }
        }
        // M[q][t] = P[ulist[t]][j_q]
        uint32_t row[8];
        {
            const U4 u0 = *reinterpret_cast<const U4 *>(ulist), u1 = *reinterpret_cast<const U4 *>(ulist + 16);
            const uint32_t uw[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
#pragma unroll
            for (int j = 0; j < 8; j++) {
                uint32_t w = 0;
#pragma unroll
                for (int bb = 0; bb < 4; bb++) {
                    const int t = j * 4 + bb;
                    if (t < r) w |= (uint32_t)ex[lgPj[(uw[j] >> (8 * bb)) & 0xFFu]] << (8 * bb);
                }
                row[j] = w;
            }
        }
        // Gauss-Jordan on [M | b]
        uint32_t dlog = 0;
#pragma unroll
        for (int col = 0; col < 32; col++) {
            if (col < r) {
                const uint32_t my = (row[col >> 2] >> (8 * (col & 3))) & 0xFFu;
                const uint32_t lgmy = lg16[my];
                const uint64_t cand = __ballot(rowl && lane >= col && my != 0);
                if (cand) {   // always true for an MDS generator
                    const int p = __ffsll((long long)cand) - 1;
                    const uint32_t lgpiv = (uint32_t)__builtin_amdgcn_readlane((int)lgmy, p);
                    uint32_t prow[8];
#pragma unroll
                    for (int j = col >> 2; j < 8; j++) prow[j] = (uint32_t)__builtin_amdgcn_readlane((int)row[j], p);
                    const uint32_t pb = (uint32_t)__builtin_amdgcn_readlane((int)b, p);
                    bool elim = rowl && my != 0 && lane != p;
                    if (p != col) {   // swap rows col <-> p (:78-90): lane col takes the pivot row, lane p the old row col
                        const uint32_t cb = (uint32_t)__builtin_amdgcn_readlane((int)b, col);
#pragma unroll
                        for (int j = col >> 2; j < 8; j++) {
                            const uint32_t cr = (uint32_t)__builtin_amdgcn_readlane((int)row[j], col);
                            if (lane == p) row[j] = cr;
                            if (lane == col) row[j] = prow[j];
                        }
                        if (lane == p) b = cb;
                        if (lane == col) b = pb;
                        elim = elim && lane != col;   // old row col had a zero here, and it now sits in lane p
                    }
                    if (lane == col) dlog = lgpiv;
                    if (elim) {
                        int lq = (int)lgmy - (int)lgpiv;
                        lq += lq < 0 ? 255 : 0;
                        const MulTab t = lds_multab(mtl, (uint32_t)lq);
#pragma unroll
                        for (int j = col >> 2; j < 8; j++) row[j] ^= gfmul4(t, prow[j]);
                        b ^= gfmul4(t, pb);
                    }
                }
            }
        }
        // x_q = b_q / d_q ; Msg(missing) = x, Msg(received source positions) = received values
        if (rowl) {
            const uint32_t bq = b & 0xFFu;
            out[ulist[lane]] = bq ? ex[(uint32_t)lg16[bq] + 255u - dlog] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (id[u] < (uint32_t)k) out[id[u]] = (uint8_t)vv[u];
    }
}

// ---- packets (S a multiple of 256), n - k <= 32, k <= 256: one WAVEFRONT per (block, 64 * 4 * VW byte slice) -------------
// The paper's system model runs "S encoders and decoders in parallel" on S-byte packets (Latex/Milcom_2022_ErasureCodes.tex:53,125);
// the elimination PATTERN (which rows, which multipliers) depends only on the received positions, the payload rides along:
//   pattern   the r x r system of the missing source symbols is inverted ONCE per block on bytes, in registers, by the same
//             Gauss-Jordan as rs_decode_s1_kernel (lane q owns row q of [M | I], first-non-zero pivoting like
//             My_RS_Decode_Optimize_With_GFTables.m:70-90): lane u ends up with row u of M^-1;
//   stream    every received row is read from HBM exactly ONCE: a received source row is written to its place in Msg and,
//             still in registers, multiplied into the r right-hand-side accumulators  b_q += P[idx_t][j_q] * v_t  (:55-67 does
//             the same elimination of the repair rows against the identity block); the accumulators -- r x 4 VW dwords per
//             lane -- live in REGISTERS (the work is dense: r multiply-accumulates per row, no LDS traffic for them), the
//             three byte-select index words of a row are built once and reused by all r products;
//   solve     x_u = sum_q M^-1[u][q] b_q  (the back substitution :100-105), written to the missing positions of Msg.
// MDS => the solution is unique => the bytes are the reference's for every decodable block.  Work per block row: r GF(256)
// multiply-accumulates (r = 25 of 223 at 10 % erasures), so the kernel is bound by vector-ALU issue, not by HBM (DESIGN.md).
struct RsPkLds {
    int pt, lg, mtl, wave0, wstride;   // P^T bytes [R][k] | log u8[256] (log 0 = 255) | multiply tables by log [256][8] (row 255 = 0) | per wave: sidx u16[256], pres u8[256], ulist u8[32]
};

template <bool NT>
__device__ __forceinline__ void rs_load_row(const uint8_t *p, uint32_t (&v)[1]) { v[0] = NT ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p)) : *reinterpret_cast<const uint32_t *>(p); }
template <bool NT>
__device__ __forceinline__ void rs_load_row(const uint8_t *p, uint32_t (&v)[2])
{
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    v[0] = __builtin_nontemporal_load(q); v[1] = __builtin_nontemporal_load(q + 1);
}
template <bool NT>
__device__ __forceinline__ void rs_load_row(const uint8_t *p, uint32_t (&v)[4])
{
    const U4 t = stream_load16<NT>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <bool NT>
__device__ __forceinline__ void rs_store_row(uint8_t *p, const uint32_t (&v)[1]) { __builtin_nontemporal_store(v[0], reinterpret_cast<uint32_t *>(p)); }
template <bool NT>
__device__ __forceinline__ void rs_store_row(uint8_t *p, const uint32_t (&v)[2])
{
    uint32_t *q = reinterpret_cast<uint32_t *>(p);
    __builtin_nontemporal_store(v[0], q); __builtin_nontemporal_store(v[1], q + 1);
}
template <bool NT>
__device__ __forceinline__ void rs_store_row(uint8_t *p, const uint32_t (&v)[4]) { stream_store16<NT>(p, U4{v[0], v[1], v[2], v[3]}); }

// FRAMES: the row of received symbol t is read in place at frame + idx_t * S.  idx_t is wave-uniform, so it goes through
// v_readfirstlane and the row address is a scalar 24-bit multiply-add (idx < n <= 255, S < 2^23 checked at launch: the product fits 32 bits) -- the
// stream loop is bound by vector-ALU issue and must not get address arithmetic on top.
template <int VW, int WPS, bool FRAMES = false>   // WPS: wavefronts per SIMD the register allocation must allow
__global__ __launch_bounds__(256, WPS) void rs_decode_packets_kernel(RsArgs a, RsPkLds L, int nslices)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int RMAX = 32;
    const int k = a.k, R = a.n - a.k, S = a.S;
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int lane = lane_id(), wave = wave_id(), nw = nthr >> 6;
    uint8_t *ptl = smem + L.pt;
    uint8_t *lg = smem + L.lg;
    uint32_t *mtl = reinterpret_cast<uint32_t *>(smem + L.mtl);
    unsigned char *wbase = smem + L.wave0 + wave * L.wstride;
    uint16_t *sidx = reinterpret_cast<uint16_t *>(wbase);
    uint8_t *pres = wbase + 512, *ulist = wbase + 768;

    for (int i = tid; i < R * k; i += nthr) ptl[i] = a.pt[i];
    for (int i = tid; i < 256; i += nthr) lg[i] = i ? c_log[i] : (uint8_t)255;
    for (int i = tid; i < 2048; i += nthr) mtl[i] = (i >> 3) < 255 ? c_mul3[(uint32_t)c_exp[i >> 3] * 8 + (i & 7)] : 0u;
    __syncthreads();

    const uint64_t lt = (1ull << lane) - 1ull;
    const int64_t nitems = a.nblocks * nslices;
    for (int64_t item = (int64_t)blockIdx.x * nw + wave; item < nitems; item += (int64_t)gridDim.x * nw) {
        const int64_t blk = item / nslices;
        const int sl = (int)(item - blk * nslices);
        const uint16_t *idx = a.recv_idx + blk * k;
        // (word form, S a multiple of 4 and not of 16, VW = 1: ceil(S / 256) slices, the last one moved back to end with the row -- where 256 VW
        // divides S the min changes nothing.  Every access of this kernel is a dword one already; a slice reads received rows and writes
        // its own bytes of msg, so the bytes two slices share are written twice with the same values and never read back)
        const uint32_t loff = min((uint32_t)sl * (uint32_t)(256 * VW), (uint32_t)(S - 256 * VW)) + (uint32_t)lane * (uint32_t)(4 * VW);
        const uint8_t *val = a.recv_val + blk * (int64_t)(FRAMES ? a.n : k) * S + loff;
        uint8_t *out = a.msg + blk * (int64_t)k * S + loff;
        uint32_t id[4];
        int nsys = 0;
        wave_sync();
        if constexpr (FRAMES) {
            if (a.nrecv[blk] < k) {   // short block (wave-uniform): zeros, no solve
                const uint32_t z[VW] = {};
                for (int t = 0; t < k; t++) rs_store_row<true>(out + (size_t)t * S, z);
                continue;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = u * 64 + lane;
            id[u] = t < k ? (uint32_t)idx[t] : 0xFFFFu;
            pres[t] = 0;
        }
        {   // positions must be < n and strictly ascending (ReedSolomonErasureCodes.m:80-81); a malformed block decodes to zeros
            bool bad = false;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int t = u * 64 + lane;
                if (t < k) bad = bad || id[u] >= (uint32_t)a.n || (t > 0 && (uint32_t)idx[t - 1] >= id[u]);
            }
            if (__ballot(bad)) {   // wave-uniform
                const uint32_t z[VW] = {};
                for (int t = 0; t < k; t++) rs_store_row<true>(out + (size_t)t * S, z);
                if (lane == 0 && sl == 0 && a.bad) atomicAdd(a.bad, 1);
                continue;
            }
        }
        wave_sync();
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = u * 64 + lane;
            const bool sys = id[u] < (uint32_t)k;      // num_sys_symbols = length(find(recv_vec_ind <= k))   (:29)
            if (sys) pres[id[u]] = 1;
            sidx[t] = (uint16_t)id[u];
            nsys += __popcll(__ballot(sys));
        }
        wave_sync();
        const int r = k - nsys;
        {   // the missing source positions, ascending
            int cnt = 0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = u * 64 + lane;
                const bool miss = (i < k) && !pres[i];
                const uint64_t mask = __ballot(miss);
                if (miss) ulist[cnt + __popcll(mask & lt)] = (uint8_t)i;
                cnt += __popcll(mask);
            }
        }
        wave_sync();
        const bool rowl = lane < r;
        const int jq = rowl ? (int)sidx[nsys + lane] - k : 0;
        const uint8_t *ptj = ptl + jq * k;
        // ---- pattern: [M | I] -> [diag | rows], lane q owns row q.  M[q][t] = P[ulist[t]][j_q]
        uint32_t row[8], irow[8];
        {
            const U4 u0 = *reinterpret_cast<const U4 *>(ulist), u1 = *reinterpret_cast<const U4 *>(ulist + 16);
            const uint32_t uw[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
#pragma unroll
            for (int j = 0; j < 8; j++) {
                uint32_t w = 0;
#pragma unroll
                for (int bb = 0; bb < 4; bb++) {
                    const int t = j * 4 + bb;
                    if (t < r) w |= (uint32_t)ptj[(uw[j] >> (8 * bb)) & 0xFFu] << (8 * bb);
                }
                row[j] = rowl ? w : 0u;
                irow[j] = ((lane >> 2) == j && rowl) ? (1u << (8 * (lane & 3))) : 0u;
            }
        }
        uint32_t dlog = 0;
#pragma unroll
        for (int col = 0; col < RMAX; col++) {
            if (col < r) {
                const uint32_t my = (row[col >> 2] >> (8 * (col & 3))) & 0xFFu;
                const uint32_t lgmy = lg[my];
                const uint64_t cand = __ballot(rowl && lane >= col && my != 0);
                if (cand) {   // always true for an MDS generator
                    const int p = __ffsll((long long)cand) - 1;
                    const uint32_t lgpiv = (uint32_t)__builtin_amdgcn_readlane((int)lgmy, p);
                    uint32_t prow[8], pirow[8];
#pragma unroll
                    for (int j = col >> 2; j < 8; j++) prow[j] = (uint32_t)__builtin_amdgcn_readlane((int)row[j], p);
#pragma unroll
                    for (int j = 0; j < 8; j++) pirow[j] = (uint32_t)__builtin_amdgcn_readlane((int)irow[j], p);
                    bool elim = rowl && my != 0 && lane != p;
                    if (p != col) {   // swap rows col <-> p (:78-90): lane col takes the pivot row, lane p the old row col
#pragma unroll
                        for (int j = col >> 2; j < 8; j++) {
                            const uint32_t cr = (uint32_t)__builtin_amdgcn_readlane((int)row[j], col);
                            if (lane == p) row[j] = cr;
                            if (lane == col) row[j] = prow[j];
                        }
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            const uint32_t ci = (uint32_t)__builtin_amdgcn_readlane((int)irow[j], col);
                            if (lane == p) irow[j] = ci;
                            if (lane == col) irow[j] = pirow[j];
                        }
                        elim = elim && lane != col;   // old row col had a zero here, and it now sits in lane p
                    }
                    if (lane == col) dlog = lgpiv;
                    if (elim) {
                        int lq = (int)lgmy - (int)lgpiv;
                        lq += lq < 0 ? 255 : 0;
                        const MulTab t = lds_multab(mtl, (uint32_t)lq);
#pragma unroll
                        for (int j = col >> 2; j < 8; j++) row[j] ^= gfmul4(t, prow[j]);
#pragma unroll
                        for (int j = 0; j < 8; j++) irow[j] ^= gfmul4(t, pirow[j]);
                    }
                }
            }
        }
        // lgi: log of every byte of row u of M^-1 = irow / d_u (255 = the entry is zero -> the all-zero table)
        uint32_t lgi[8];
        {
            const uint32_t linv = dlog ? 255u - dlog : 0u;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                uint32_t w = 0;
#pragma unroll
                for (int bb = 0; bb < 4; bb++) {
                    const uint32_t b = (irow[j] >> (8 * bb)) & 0xFFu;
                    uint32_t l = (uint32_t)lg[b] + linv;
                    l = l >= 255u ? l - 255u : l;
                    w |= (b ? l : 255u) << (8 * bb);
                }
                lgi[j] = w;
            }
        }

        // ---- stream + solve, instantiated for Q = 4, 8, ... 32 accumulators (r rounded up to a multiple of four: the padding
        //      lanes carry log 255 = the all-zero table, so they add nothing).  Straight-line code over the accumulators: the
        //      compiler pipelines the table reads of one product behind the byte selects of the previous ones.
        auto data_phase = [&](auto qtag) {
            constexpr int Q = decltype(qtag)::value;
            // accumulators start as the received repair rows (b_q = c_{j_q} + ...); then every received source row is copied
            // to Msg and multiplied into them
            uint32_t acc[Q][VW];
#pragma unroll
            for (int q = 0; q < Q; q++) {
#pragma unroll
                for (int d = 0; d < VW; d++) acc[q][d] = 0u;
                if constexpr (FRAMES) { if (q < r) rs_load_row<true>(val + __umul24(uniform((uint32_t)sidx[nsys + q]), (uint32_t)S), acc[q]); }
                else if (q < r) rs_load_row<true>(val + (size_t)(nsys + q) * S, acc[q]);
            }
            uint32_t vcur[VW], vnxt[VW];
#pragma unroll
            for (int d = 0; d < VW; d++) vcur[d] = vnxt[d] = 0u;
            uint32_t itc = 0;   // FRAMES: position of the row in vcur (scalar)
            if constexpr (FRAMES) {
                if (nsys > 0) { itc = uniform((uint32_t)sidx[0]); rs_load_row<true>(val + __umul24(itc, (uint32_t)S), vcur); }
            } else if (nsys > 0) rs_load_row<true>(val, vcur);
            for (int t = 0; t < nsys; t++) {
                // (clamped: the row past the end is the last one again -- an unconditional load keeps the loop branch-free)
                uint32_t it;
                if constexpr (FRAMES) {
                    const uint32_t itn = uniform((uint32_t)sidx[t + 1 < nsys ? t + 1 : t]);
                    rs_load_row<true>(val + __umul24(itn, (uint32_t)S), vnxt);
                    it = itc; itc = itn;
                } else {
                    rs_load_row<true>(val + (size_t)(t + 1 < nsys ? t + 1 : t) * S, vnxt);
                    it = (uint32_t)sidx[t];              // wave-uniform
                }
                const uint32_t lgc = rowl ? (uint32_t)lg[ptj[it]] : 255u;   // lane q: log P[idx_t][j_q]
                rs_store_row<true>(out + (size_t)it * S, vcur);
                Sel3 sel[VW];
#pragma unroll
                for (int d = 0; d < VW; d++) sel[d] = gfsel(vcur[d]);
                // the multiply tables of product q + PF are requested before product q is computed (static register rotation)
                constexpr int PF = 3;
                MulTab tq[PF + 1];
#pragma unroll
                for (int q = 0; q < PF && q < Q; q++) tq[q] = lds_multab(mtl, (uint32_t)__builtin_amdgcn_readlane((int)lgc, q));
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    if (q + PF < Q) tq[(q + PF) % (PF + 1)] = lds_multab(mtl, (uint32_t)__builtin_amdgcn_readlane((int)lgc, q + PF));
                    __builtin_amdgcn_sched_barrier(0);
                    const MulTab &tb = tq[q % (PF + 1)];
#pragma unroll
                    for (int d = 0; d < VW; d++) acc[q][d] = gfmac4_sel(acc[q][d], tb, sel[d]);
                }
#pragma unroll
                for (int d = 0; d < VW; d++) vcur[d] = vnxt[d];
            }
            // solve: x_u = sum_q M^-1[u][q] b_q, written to the missing source positions
            for (int u = 0; u < r; u++) {
                uint32_t x[VW];
#pragma unroll
                for (int d = 0; d < VW; d++) x[d] = 0u;
                constexpr int PF = 3;
                MulTab tq[PF + 1];
                auto tab_of = [&](int q) {
                    const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)lgi[q >> 2], u);
                    return lds_multab(mtl, (w >> (8 * (q & 3))) & 0xFFu);
                };
#pragma unroll
                for (int q = 0; q < PF && q < Q; q++) tq[q] = tab_of(q);
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    if (q + PF < Q) tq[(q + PF) % (PF + 1)] = tab_of(q + PF);
                    __builtin_amdgcn_sched_barrier(0);
                    const MulTab &tb = tq[q % (PF + 1)];
#pragma unroll
                    for (int d = 0; d < VW; d++) x[d] = gfmac4_sel(x[d], tb, gfsel(acc[q][d]));
                }
                rs_store_row<true>(out + (size_t)ulist[u] * S, x);
            }
        };
        switch ((r + 3) >> 2) {
            case 0: case 1: data_phase(std::integral_constant<int, 4>{}); break;
            case 2: data_phase(std::integral_constant<int, 8>{}); break;
            case 3: data_phase(std::integral_constant<int, 12>{}); break;
            case 4: data_phase(std::integral_constant<int, 16>{}); break;
            case 5: data_phase(std::integral_constant<int, 20>{}); break;
            case 6: data_phase(std::integral_constant<int, 24>{}); break;
            case 7: data_phase(std::integral_constant<int, 28>{}); break;
            default: data_phase(std::integral_constant<int, 32>{}); break;
        }
    }
}

// codeword = source * G, G = [I | P]   (Matlab/Test_My_RS_Decode.m:48)
__global__ __launch_bounds__(256) void rs_encode_kernel(int n, int k, int S, int64_t nblocks, const uint8_t *pt,
                                                        const uint8_t *src, uint8_t *cw)
{
    const int lane = lane_id(), wave = wave_id(), nw = (int)(blockDim.x >> 6);
    const int R = n - k;
    for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const uint8_t *s = src + blk * (int64_t)k * S;
        uint8_t *c = cw + blk * (int64_t)n * S;
        if (S == 1) {
            for (int i = (int)threadIdx.x; i < k; i += (int)blockDim.x) c[i] = s[i];
            for (int j = wave; j < R; j += nw) {
                uint32_t acc = 0;
                for (int i = lane; i < k; i += kWave) acc ^= gfmul_log(c_log, c_exp, pt[(size_t)j * k + i], s[i]);
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) acc ^= __shfl_xor(acc, d);
                if (lane == 0) c[k + j] = (uint8_t)acc;
            }
        } else {
            const bool w4 = (S & 15) != 0;   // word form: dword copy, ceil(S / 16) chunks with the last one moved back (rs_decode_kernel)
            const int chunks = (S + 15) >> 4;
            if (w4) {
                for (int64_t u = threadIdx.x; u < (int64_t)k * (S >> 2); u += blockDim.x)
                    reinterpret_cast<uint32_t *>(c)[u] = reinterpret_cast<const uint32_t *>(s)[u];
            } else {
                for (int64_t u = threadIdx.x; u < (int64_t)k * chunks; u += blockDim.x)
                    reinterpret_cast<U4 *>(c)[u] = reinterpret_cast<const U4 *>(s)[u];
            }
            for (int j = wave; j < R; j += nw)
                for (int i = lane; i < chunks; i += kWave) {
                    const int off = w4 ? min(i * 16, S - 16) : i * 16;
                    U4 acc = {0, 0, 0, 0};
                    for (int t = 0; t < k; t++) {
                        const U4 v = rs_ld16(s + (size_t)t * S + off, w4);
                        gfmac16(acc, load_multab(uniform(pt[(size_t)j * k + t])), v);
                    }
                    rs_st16(c + (size_t)(k + j) * S + off, acc, w4);
                }
        }
    }
}
