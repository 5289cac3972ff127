// ml_kernel.inc -- hybrid ML stage (a2-a4) for the residual frames (included by kernels.hip).
//
// Reference: Matlab/My_LDPC_HybridML_NonBinary_Erasure_Decoder.m:61-128.  One workgroup per residual frame (frames are
// handed out through a device counter, so long eliminations do not queue behind each other).
//
// Exactness: the reference picks as pivot the FIRST row >= col with a non-zero in column col (:86), swaps it to row
// col (:92-97), scales it by the inverse of its leading entry (:99-105), eliminates only the rows BELOW (:107-114),
// stops on an empty column (:87-90) but still writes rhs(1:E) back (:127).  The kernel executes the same sequence of
// field operations in a form that needs ONE workgroup barrier per column:
//   * rows are never moved: `perm` (logical row -> stored row) and `iperm` record the reference's swaps, and the pivot
//     search minimises the LOGICAL index, so the pivot order is the reference's;
//   * the pivot row is not scaled in place: the row update uses the factor f * inv(pivot) on the unscaled pivot row
//     (GF(256) products are exact and associative, so every byte equals the reference's), and log(inv(pivot)) is kept
//     per column (`plog`) and applied when a pivot row's right-hand side is read (back substitution, write-back);
//   * the pivot search and the non-zero row list of column col+1 are produced while column col is eliminated: the lane
//     that updates the chunk holding column col+1 of a row reports the new byte, untouched rows are read by idle
//     threads (counters triple-buffered, so no reset races with a reader);
//   * all-zero rows of H(:, erased) -- checks without an erased neighbour -- take no part in the elimination.  They are
//     not stored; `perm` still tracks where the reference's swaps put them, and their right-hand side is recomputed in
//     the one place it can be observed (the write-back of a rank-deficient frame).
// Hence rank-deficient frames come out with the reference's bytes too.
//
// Storage: the non-zero rows (nzr <= m) x W bytes, W = 16 * (odd number of chunks) so that a column walk spreads over
// the LDS banks; in LDS whenever nzr * W fits (E up to ~350 for the (2040,1530) code), else in a per-workgroup global
// scratch (same code, instantiated for the other address space).  S = 1: the right-hand side is one more chunk of every
// row.
//
// Packets (S >= 16): the elimination pattern -- pivot order, multipliers -- does not depend on the payload, and a
// per-column barrier around 1 KB row updates in global memory is a chain of 2 E dependent L2 round trips.  So the
// matrix is factored ONCE on bytes (same loop as above, LU in place: the multiplier f / pivot that zeroes A[x][col] is
// stored in that byte, which the elimination never looks at again), and the right-hand sides -- S-byte rows in global
// memory, one wavefront per row, wave-uniform multipliers -- are then solved in PULL form, level by level:
//     forward   R_x  = rhs_x + sum_{col < t_x} L[x][col] R_{perm[col]}          t_x = logical position of stored row x
//     backward  X_r  = inv(piv_r) (R_{perm[r]} + sum_{j > r} a(r,j) X_j)        X = the solved symbols, read from `out`
// a row waits only for the rows it really depends on (level = 1 + max level of its sources; about 50 + 50 levels for
// E = 230 instead of 460 column steps).  Every field operation is one the reference performs (XOR sums regrouped, products
// exact), so the bytes -- rank-deficient frames included -- are the reference's.
struct MlArgs {
    DevCode code;
    int S, Spad;
    int capA;               // bytes of LDS available for the matrix
    const int32_t *ml_list;   // layout: PeelArgs::ml_list
    int64_t nframes;          // frames of the batch (stride of the size-class lists)
    const uint8_t *ml_state;
    int32_t *work;          // device counter handing out slots of ml_list
    uint8_t *out;           // [nframes][n][S]
    uint8_t *wsA;           // [gridDim.x][m][maxrow]   global fallback for the matrix
    uint8_t *wsR;           // [gridDim.x][m][Spad]     packet right-hand sides (S > 1)
    int maxrow;
    int32_t *status;
    int lds_A, lds_colmap, lds_elist, lds_colv, lds_rlist, lds_perm, lds_iperm, lds_plog, lds_orow, lds_mt, lds_lg, lds_ex, lds_misc;
    int lds_lvl;            // u32 [m + 2]: packets -- forward level of every stored row, later the level offsets of the sort
    // packets: the solve schedule of every ML frame (see ml_emit_schedule / ldpc_ml_solve_kernel)
    unsigned long long *ops;        // arena of 64-bit words
    unsigned long long ops_cap;     // its size in words
    unsigned long long *ops_head;   // bump pointer (device counter)
    uint32_t *rec;                  // [ML-list slot][8]: arena offset lo/hi, levels, slots, ops, fall-back flag
    int use_solve;                  // 0: always solve inside this kernel (A/B knob, fall-back path)
    int solve_b;                    // bytes of every row per solve-kernel workgroup: ops carry LDS addresses of its slots
    int dbg;                        // diagnostic build only (-DLDPC_AMD_MLDBG, tools/sens_ml.py): repeat parts of the column step
    int use_pi;                     // ldpc_ml_pi_kernel ran first: frames with rec[6] != 0 already have their schedule (ml_pi.inc)
    int mode;                       // 0: everything in this launch.  1: pattern only (the launch runs beside the packet kernel): a frame
                                    // whose schedule does not fit the arena is deferred (rec[5] = 2, work[1]++).  2: the deferred frames
    int32_t *work2;                 // hand-out counter of a mode-2 launch
    int32_t *nfail, *work3;         // mode 3: the frames whose fast-path solution failed the consistency check (rec[7] = 1), factored exactly
};

constexpr uint32_t kMlNoPivot = ~0u;
constexpr uint32_t kMlSlot0 = 8192;   // LDS address of slot 0 in the solve kernel (its 8 KB of multiply tables come first)
__device__ __forceinline__ unsigned long long ml_op(uint32_t dst, uint32_t coef, uint32_t src)
{
    return (unsigned long long)(dst | (coef << 24)) | ((unsigned long long)src << 32);
}

// key of the pivot search: smallest logical row wins; the stored row and the LOG of its byte ride along.  32 bits
// (12 | 12 | 8: up to 4096 checks, checked by the host): a 32-bit LDS minimum is one ds_min_u32, where the 64-bit key of the first
// version made the compiler walk the reporting lanes one by one in a scalar loop before every ds_min_u64.
__device__ __forceinline__ uint32_t ml_key(int logical, int stored, uint32_t lgv)
{
    return ((uint32_t)logical << 20) | ((uint32_t)stored << 8) | lgv;
}

// sum over the known neighbours of original check r, one byte lane (S = 1)
__device__ __forceinline__ uint32_t ml_rhs_byte(const DevCode &cd, const uint16_t *colmap_or_null, const uint8_t *state,
                                                const uint8_t *fout, const uint8_t *lg, const uint8_t *ex, int r)
{
    uint32_t acc = 0;
    for (int t = 0; t < cd.degpad; t++) {
        const uint32_t col = cd.ell_col[(size_t)t * cd.mpad + r];
        if (col == 0xFFFFu) break;
        const bool erased = colmap_or_null ? (colmap_or_null[col] != 0xFFFFu) : (state[col] != 0);
        if (erased) continue;
        const uint32_t v = fout[col];
        if (v) acc ^= ex[(uint32_t)cd.ell_logc[(size_t)t * cd.mpad + r] + lg[v]];
    }
    return acc;
}

// W4 (packets only; ldpc_ml_words_kernel): S is a multiple of 4, not of 16 -- the rows of `out` start on 4-byte boundaries and the
// last 16-byte chunk of a row would cross its end.  A lane's chunk i then lies at min(16 i, S - 16): the last chunk is moved back to
// end with the row and shares bytes with the one before it.  The scratch rows R keep the chunk index (stride Spad = S rounded up to
// 16, 16-byte accesses), so chunk i of a scratch row always belongs to the same bytes of the symbols.  Both lanes of an overlap compute
// the same values (the arithmetic is columnwise) and store them twice; every row of `out` that is read here was either received (the
// packet kernel wrote it, an earlier launch) or written by a wavefront of an EARLIER level, with a workgroup barrier in between.
template <bool IN_LDS, bool PK, bool W4 = false>   // PK: packets (S != 1) -- LU in place, forward levels, solve-schedule emission
__device__ __forceinline__ void ml_frame(const MlArgs &a, const int64_t f, const int slot, const uint8_t *state, const int E,
                                         const int nzr, const int nch, const int ach)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const DevCode &cd = a.code;
    const int n = cd.n, m = cd.m, S = a.S;
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int lane = lane_id(), wave = wave_id(), nw = nthr >> 6;
    const int W = nch << 4;
    const int ro = ach << 4;                                   // S == 1: byte offset of the rhs inside a row
    const int rch = a.Spad >> 4;
    auto fo = [&](int i) { return W4 ? min(i * 16, S - 16) : i * 16; };   // byte offset of chunk i in a row of `out`

    uint16_t *colmap = reinterpret_cast<uint16_t *>(smem + a.lds_colmap);   // build phase only (aliases rlist[1..2])
    uint16_t *elist = reinterpret_cast<uint16_t *>(smem + a.lds_elist);
    uint8_t *colv = smem + a.lds_colv;                                        // [3][mpad]
    uint32_t *rlist = reinterpret_cast<uint32_t *>(smem + a.lds_rlist);      // [3][m]
    uint16_t *perm = reinterpret_cast<uint16_t *>(smem + a.lds_perm);        // logical -> stored row, or 0x8000 | check
    uint16_t *iperm = reinterpret_cast<uint16_t *>(smem + a.lds_iperm);      // stored row -> logical
    uint8_t *plog = smem + a.lds_plog;                                        // column -> log(inv(pivot))
    uint16_t *orow = reinterpret_cast<uint16_t *>(smem + a.lds_orow);        // stored row -> check
    const uint32_t *mt = reinterpret_cast<const uint32_t *>(smem + a.lds_mt);   // multiply tables indexed by LOG(coefficient)
    const uint8_t *lg = smem + a.lds_lg, *ex = smem + a.lds_ex;               // ex has 1024 entries
    int *misc = reinterpret_cast<int *>(smem + a.lds_misc);
    uint32_t *key = reinterpret_cast<uint32_t *>(smem + a.lds_misc + 64);  // [3]
    int *cnt = misc + 4;                                                      // [3]
    int *pcbuf = misc + 8;                                                    // [3] row stored at logical col (or 0x8000|check)

    uint32_t *lvl = reinterpret_cast<uint32_t *>(smem + a.lds_lvl);             // packets: forward level of every stored row
    constexpr bool pk = PK;

    uint8_t *A = IN_LDS ? (smem + a.lds_A) : (a.wsA + (size_t)blockIdx.x * m * a.maxrow);
    uint8_t *R = a.wsR + (size_t)blockIdx.x * m * a.Spad;     // packets only, indexed by stored row
    uint8_t *fout = a.out + f * (int64_t)n * S;
    const int mp = cd.mpad;

#ifdef LDPC_AMD_STAMPS
    unsigned long long ml_prev = __builtin_amdgcn_s_memtime();
#define ML_STAMP(i) do { if (tid == 0) { const unsigned long long t__ = __builtin_amdgcn_s_memtime(); atomicAdd(&g_peel_stamps[16 + (i)], t__ - ml_prev); ml_prev = t__; } } while (0)
#else
#define ML_STAMP(i) do { } while (0)
#endif
    // ---- zero the stored rows, then scatter H(:, erased) into them (:65) and build the right-hand sides (:74-82)
    for (int i = tid; i < nzr * nch; i += nthr) *reinterpret_cast<U4 *>(A + (size_t)i * 16) = U4{0, 0, 0, 0};
    if (pk) {
        for (int c = tid; c < nzr; c += nthr) lvl[c] = 0u;
        if (tid == 0) misc[12] = 0;
    }
    __syncthreads();
    for (int c = tid; c < nzr; c += nthr) {
        const int r = orow[c];
        uint32_t acc = 0, v0 = 0;
        for (int t = 0; t < cd.degpad; t++) {
            const uint32_t col = cd.ell_col[(size_t)t * mp + r];
            if (col == 0xFFFFu) break;
            const uint32_t cm = colmap[col];
            if (cm != 0xFFFFu) {
                const uint8_t coef = cd.ell_coef[(size_t)t * mp + r];
                A[(size_t)c * W + cm] = coef;
                if (cm == 0) v0 = coef;
            } else if (!PK) {
                const uint32_t v = fout[col];
                if (v) acc ^= ex[(uint32_t)cd.ell_logc[(size_t)t * mp + r] + lg[v]];
            }
        }
        if (!PK) A[(size_t)c * W + ro] = (uint8_t)acc;
        colv[c] = (uint8_t)v0;
        if (v0) {
            const uint32_t l0 = lg[v0];
            atomicMin(&key[0], ml_key(r, c, l0));
            rlist[atomicAdd(&cnt[0], 1)] = (uint32_t)c | (l0 << 16);
        }
    }
    // packets, in-kernel solve only (the fall-back when the solve schedule cannot be emitted): right-hand sides of the stored
    // rows as S-byte rows in the workgroup's global scratch
    auto build_packet_rhs = [&]() {
        for (int c = wave; c < nzr; c += nw) {
            const int r = orow[c];
            // lane t looks at edge t of the check; the known neighbours are then walked 8 at a time with their row loads
            // issued back to back (the rows come from HBM: the packet kernel stored them non-temporally)
            uint32_t colL = 0xFFFFu, cfL = 0;
            if (lane < cd.degpad) {
                colL = cd.ell_col[(size_t)lane * mp + r];
                cfL = cd.ell_coef[(size_t)lane * mp + r];
            }
            const bool knownL = colL != 0xFFFFu && state[colL] == 0;   // (colmap is dead by now)
            const uint64_t kmask = __ballot(knownL);
            for (int i = lane; i < ((rch + kWave - 1) & ~(kWave - 1)); i += kWave) {
                const bool act = i < rch;
                U4 acc = {0, 0, 0, 0};
                uint64_t km = kmask;
                while (km) {
                    U4 v[8];
                    uint32_t cf[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        cf[u] = 0;
                        v[u] = U4{0, 0, 0, 0};
                        if (km) {
                            const int e = __ffsll((long long)km) - 1;
                            km &= km - 1;
                            const uint32_t col = (uint32_t)__builtin_amdgcn_readlane((int)colL, e);
                            cf[u] = (uint32_t)__builtin_amdgcn_readlane((int)cfL, e);
                            if (act) v[u] = row_load16<W4>(fout + (int64_t)col * S + fo(i));
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        if (cf[u]) gfmac16(acc, load_multab(cf[u]), v[u]);
                }
                if (act) *reinterpret_cast<U4 *>(R + (size_t)c * a.Spad + i * 16) = acc;
            }
        }
    };

#ifdef LDPC_AMD_MLDBG
    // floors of a column step (diagnostic build only): E extra steps that are nothing but the barrier and the header read
    // (4096), plus a row update by every lane group on a row of its own (8192), before the real loop
    if (a.dbg & (4096 | 8192)) {
        uint32_t sink = 0;
        for (int col = 0; col < E; col++) {
            __syncthreads();
            const uint32_t K = key[col % 3];
            const int nel = cnt[col % 3];
            sink += uniform(K) + uniform((uint32_t)nel);
            if (a.dbg & 8192) {
                const int x = (tid >> 4) % nzr, ci = tid & 15;
                if (ci < nch) {
                    const MulTab t = lds_multab(mt, (uint32_t)((col + tid) & 127));
                    U4 v = *reinterpret_cast<const U4 *>(A + (size_t)x * W + ci * 16);
                    const U4 pv = *reinterpret_cast<const U4 *>(A + (size_t)((x + 1) % nzr) * W + ci * 16);
                    gfmac16(v, t, pv);
                    if (v.x == 0x12345678u && v.y == 0x9ABCDEF0u) misc[31] = 1;
                }
            }
        }
        if (sink == 0x12345u) misc[31] = 1;
        __syncthreads();
    }
#endif
    ML_STAMP(0);
    // ---- forward elimination (:85-115), one barrier per column
    int brk = -1;
    const int first_scan_wave = max(0, (nthr - nzr) >> 6);   // wavefronts whose threads take part in the untouched-row scan
    int b = 0, b1 = 1, b2 = 2;   // col % 3, (col + 1) % 3, (col + 2) % 3, rotated (every wavefront runs this header E times)
    for (int col = 0; col < E; col++, b = b1, b1 = b2, b2 = 3 - b - b1) {
        const int c0 = col >> 4;
        // lanes per row: the power of two covering the chunks right of the pivot column
        const int nact = nch - c0;
        const int lsh = nact <= 1 ? 0 : min(6, 32 - __builtin_clz((unsigned)(nact - 1)));   // ceil(log2(nact)), at most 6
        const int gpw = 64 >> lsh;
        __syncthreads();
#ifdef LDPC_AMD_MLDBG
        if (a.dbg & 2) __syncthreads();
#endif
        ML_STAMP(1);
        // everything a lane needs first is requested in one go: the pivot key, the list length, its first list entry
        const uint32_t K = key[b];
        const int nel = cnt[b];
        if (K == kMlNoPivot) { brk = col; break; }                 // :87-90
#ifdef LDPC_AMD_MLDBG
        if ((a.dbg & 16) && col == 0) { brk = 0; break; }          // no column at all: what the rest of the kernel costs
        if ((a.dbg & 32) && col == E / 2) { brk = col; break; }     // half of the columns
#endif
        // A column step has work for the wavefronts that update rows (the first ceil(nel / gpw)), for those that scan the
        // untouched rows (the last ceil(nzr / 64)) and for the last one (bookkeeping).  The others -- a third of the
        // workgroup on a typical system -- go straight to the barrier: the kernel is bound by instruction issue (every
        // wavefront used to run the whole header: more scalar than vector instructions in the counters), not by the barrier.
        if (!(wave * gpw < nel || wave >= first_scan_wave)) continue;
        const bool has_next = col + 1 < E;
        const int cn = (col + 1) >> 4, sn = ((col + 1) & 3) * 8, wn = ((col + 1) >> 2) & 3;
        const uint8_t *cvb = colv + b * mp;
        uint8_t *cvn = colv + b1 * mp;
        const uint32_t *rlb = rlist + b * m;
        uint32_t *rln = rlist + b1 * m;
        const int lpg = 1 << lsh;
        const int g = lane >> lsh, gl = lane & (lpg - 1);
        const int ngroups = nw * gpw, gid = wave * gpw + g;
        const int pcw = pcbuf[b];
        const uint32_t ent0 = rlb[gid < m ? gid : 0];
        const int p = (int)(K >> 20), pp = (int)((K >> 8) & 0xFFFu);
        const int pc = (pcw & 0x8000) ? -1 : pcw;
        const uint32_t lgp = (uint32_t)(K & 0xFFu);
        const uint32_t lpi = lgp ? 255u - lgp : 0u;                  // log(inv(pivot)) = (255 - log pivot) mod 255
        // packets: L[x][col] = f / pivot is stored in the byte the elimination zeroes.  The pivot row's own multipliers sit
        // in the bytes left of column col of chunk c0: they must not be added to the rows below (cmask keeps bytes >= cb).
        const int cb = col & 15;
        uint32_t lvl_pp = 0u;
        uint32_t cm[4] = {0u, 0u, 0u, 0u};
        if (pk && gid < nel) {   // only the lanes that update a row need these
            lvl_pp = lvl[pp];
#pragma unroll
            for (int d = 0; d < 4; d++) cm[d] = d < (cb >> 2) ? 0u : (d == (cb >> 2) ? (0xFFFFFFFFu << ((cb & 3) * 8)) : 0xFFFFFFFFu);
        }
        if (tid == nthr - 1) {   // the reference's swap (:92-97) as an exchange of two map entries; :99-105 kept as a log
            perm[col] = (uint16_t)pp; perm[p] = (uint16_t)pcw;
            iperm[pp] = (uint16_t)col;
            if (pc >= 0) iperm[pc] = (uint16_t)p;
            plog[col] = (uint8_t)lpi;
            pcbuf[b1] = (col + 1 < m) ? perm[col + 1] : 0;
            key[b2] = kMlNoPivot; cnt[b2] = 0;
#ifdef LDPC_AMD_MLDBG
            if (a.dbg & 128) {   // four dependent LDS round trips more on the bookkeeping thread
                uint32_t d = lpi;
                for (int q = 0; q < 4; q++) d = ex[(d & 255u) + q];
                if (d == 0x12345u) misc[31] = 1;
            }
#endif
        }
#ifdef LDPC_AMD_MLDBG
        if (a.dbg & 256) {   // four dependent LDS round trips more in every wavefront's header
            uint32_t d = lpi;
            for (int q = 0; q < 4; q++) d = ex[(d & 255u) + q];
            if (d == 0x12345u) misc[31] = 1;
        }
#endif

        ML_STAMP(2);
        // zero the rows below that have a non-zero in this column (:107-114); rows are independent
        for (int i = gid; i < nel; i += ngroups) {
            const uint32_t ent = (i == gid) ? ent0 : rlb[i];
            const int x = (int)(ent & 0xFFFFu);
            if (x == pp) continue;
            uint32_t lf = (ent >> 16) + lpi;                       // log(f * inv(pivot))
            lf = lf >= 255u ? lf - 255u : lf;
            const MulTab t = lds_multab(mt, lf);
            uint8_t *rx = A + __umul24((uint32_t)x, (uint32_t)W);   // (24-bit multiply: full rate; x < 4096, W < 8192)
            const uint8_t *rp = A + (size_t)pp * W;
            const uint32_t gsh = pk ? ((uint32_t)ex[lf] << ((cb & 3) * 8)) : 0u;   // the multiplier, at byte cb of its dword
#ifdef LDPC_AMD_MLDBG
            if (a.dbg & 8) {   // four dependent LDS round trips more on the row-update chain
                uint32_t d = lf;
                for (int q = 0; q < 4; q++) d = ex[(d & 255u) + q];
                if (d == 0x12345u) misc[31] = 1;
            }
            if (a.dbg & 4) {   // the row update once more, into nowhere
                for (int ci = c0 + gl; ci < nch; ci += lpg) {
                    U4 v = *reinterpret_cast<const U4 *>(rx + ci * 16);
                    gfmac16(v, lds_multab(mt, (lf + 1u) % 255u), *reinterpret_cast<const U4 *>(rp + ci * 16));
                    if (v.x == 0x12345678u && v.y == 0x9ABCDEF0u) misc[31] = 1;
                }
            }
#endif
            for (int ci = c0 + gl; ci < nch; ci += lpg) {
                U4 v = *reinterpret_cast<const U4 *>(rx + ci * 16);
                U4 pv = *reinterpret_cast<const U4 *>(rp + ci * 16);
                if (pk && ci == c0) { pv.x &= cm[0]; pv.y &= cm[1]; pv.z &= cm[2]; pv.w &= cm[3]; }
                gfmac16(v, t, pv);
                if (pk && ci == c0) {   // byte cb is zero now (f + (f / piv) piv): it takes the multiplier
                    const int d = cb >> 2;
                    if (d == 0) v.x |= gsh; else if (d == 1) v.y |= gsh; else if (d == 2) v.z |= gsh; else v.w |= gsh;
                }
                *reinterpret_cast<U4 *>(rx + ci * 16) = v;
                if (has_next && ci == cn) {
                    const uint32_t w4 = wn == 0 ? v.x : (wn == 1 ? v.y : (wn == 2 ? v.z : v.w));
                    const uint32_t nv = (w4 >> sn) & 0xFFu;
                    cvn[x] = (uint8_t)nv;
                    if (nv) {
                        const int l = (x == pc) ? p : (int)iperm[x];
                        const uint32_t ln = lg[nv];
                        atomicMin(&key[b1], ml_key(l, x, ln));
                        rln[atomicAdd(&cnt[b1], 1)] = (uint32_t)x | (ln << 16);
#ifdef LDPC_AMD_MLDBG
                        if (a.dbg & 64) {   // the two same-address atomics once more (dummy targets)
                            atomicMin(reinterpret_cast<uint32_t *>(misc + 26), ml_key(l, x, ln));
                            if (atomicAdd(&misc[30], 1) == 0x7FFFFFF0) misc[31] = 1;
                        }
#endif
                    }
                }
            }
            if (pk && gl == 0) atomicMax(&lvl[x], lvl_pp + 1u);   // x now waits for the pivot row (off the critical path)
        }
        ML_STAMP(3);
        // rows this column leaves untouched: their byte of column col+1 is read in place
        if (has_next) {
            for (int x = nthr - 1 - tid; x < nzr; x += nthr) {   // high threads first: the low ones eliminate
                if (x == pp) continue;
                const int l = (x == pc) ? p : (int)iperm[x];
                if (l <= col || cvb[x]) continue;
                const uint32_t nv = A[__umul24((uint32_t)x, (uint32_t)W) + (uint32_t)(col + 1)];
                cvn[x] = (uint8_t)nv;
                if (nv) {
                    const uint32_t ln = lg[nv];
                    atomicMin(&key[b1], ml_key(l, x, ln));
                    rln[atomicAdd(&cnt[b1], 1)] = (uint32_t)x | (ln << 16);
                }
            }
        }
#ifdef LDPC_AMD_MLDBG
        if ((a.dbg & 1) && has_next) {   // the scan once more, into nowhere
            for (int x = nthr - 1 - tid; x < nzr; x += nthr) {
                if (x == pp) continue;
                const int l = (x == pc) ? p : (int)iperm[x];
                if (l <= col || cvb[x]) continue;
                const uint32_t nv = A[(size_t)x * W + col + 1];
                if (nv && lg[nv] == 300u) misc[31] = 1;
            }
        }
#endif
        ML_STAMP(4);
    }
    __syncthreads();
    const int dont_do_jordan = brk >= 0;
    const int npiv = dont_do_jordan ? brk : E;
    uint32_t *steps = rlist, *sorted = rlist + m;                 // the column lists are dead from here on
    uint16_t *slvl = reinterpret_cast<uint16_t *>(colv);           // ... and so are the column bytes (3 mpad >= 2 m bytes)

    // ---- packets: emit the frame's SOLVE SCHEDULE and leave the payload to ldpc_ml_solve_kernel --------------------------
    // What is left to do with the S-byte rows is a fixed list of multiply-accumulates "slot[dst] ^= coef * source", known
    // from the factorisation alone.  It is written to a global arena as 64-bit ops, PRE-DECODED for the solve kernel (round 3:
    // its levels are bound by vector-instruction issue, and a third of an op's instructions were field extraction and address
    // arithmetic): low word = LDS address of the destination slot | coef << 24 (the solve kernel keeps its multiply tables at
    // LDS address 0, so coef * 32 = word >> 19 is the table address, and the slots behind them at kMlSlot0 + slot * B), high
    // word = LDS address of the source slot -- or the symbol index where the source (level 0) or the destination (last level) is
    // a row of `out`.  Ops are grouped
    // by dependency level; the solve kernel keeps one LDS slot of B bytes per stored row (one workgroup per B-byte slice
    // of the frame) and runs the levels with a workgroup barrier in between:
    //   level 0            slot[c] ^= h * out[symbol]        known neighbours of the stored row's check (source: global)
    //   levels 1..mxl      slot[x] ^= L[x][col] * slot[perm[col]]                         forward solve, pull form
    //   then mxb + 1       slot[perm[r]] ^= (a(r,j) / piv_j) * slot[perm[j]]              backward solve on UNSCALED rows
    //   last level         out[elist[t]] = scale_t * slot[tslot[t]]                       (:127, unconditional)
    // Rank-deficient frames have no backward levels; the all-zero rows their write-back reads get slots of their own.
    if (pk && a.use_solve && a.mode != 2) {
        uint32_t *hist = rlist;                                                        // [NL + 1], NL <= 2 m + 3
        uint16_t *tslot = reinterpret_cast<uint16_t *>(rlist + 2 * m + 4);            // logical row t < E -> slot
        // backward levels: one wavefront walks the rows from the last to the first (level = 1 + max level of the rows read)
        if (wave == 0) {
            int mxl = 0;
            for (int c0_ = 0; c0_ < nzr; c0_ += kWave) {
                const int c = c0_ + lane;
                if (c < nzr && (int)iperm[c] < E) mxl = max(mxl, (int)lvl[c]);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) mxl = max(mxl, __shfl_xor(mxl, d));
            int mxb = -1;
            if (!dont_do_jordan) {
                // bl[r] = 1 + max bl[j] over the rows j > r that row r reads (a(r,j) != 0).  Push form, no reduction: lane l
                // keeps the levels of the logical rows l, l + 64, ... in registers; column col's level is broadcast with
                // v_readlane and pushed into the rows above that have an entry in the column (fetched one column ahead).
                constexpr int NP = 8;
                mxb = 0;
                if (E <= NP * kWave) {
                    uint32_t off[NP], bl[NP];
#pragma unroll
                    for (int q = 0; q < NP; q++) {
                        const int r = q * kWave + lane;
                        off[q] = (r < E) ? (uint32_t)perm[r] * (uint32_t)W : 0u;
                        bl[q] = 0u;
                    }
                    auto fetch_col = [&](int col, uint32_t (&nz)[NP]) {
#pragma unroll
                        for (int q = 0; q < NP; q++) {
                            const int r = q * kWave + lane;
                            nz[q] = (q * kWave < col && r < col) ? (uint32_t)A[off[q] + col] : 0u;
                        }
                    };
                    uint32_t cur[NP], nxt[NP];
                    fetch_col(E - 1, cur);
#pragma unroll
                    for (int p = NP - 1; p >= 0; p--) {
                        if (p * kWave >= E) continue;
                        const int ltop = (E - 1 - p * kWave) < (kWave - 1) ? (E - 1 - p * kWave) : (kWave - 1);
                        for (int l = ltop; l >= 0; l--) {
                            const int col = p * kWave + l;
                            if (col == 0) break;
                            if (col > 1) fetch_col(col - 1, nxt);
                            const uint32_t c1 = (uint32_t)__builtin_amdgcn_readlane((int)bl[p], l) + 1u;
#pragma unroll
                            for (int q = 0; q <= p; q++)
                                if (cur[q]) bl[q] = max(bl[q], c1);
#pragma unroll
                            for (int q = 0; q < NP; q++) cur[q] = nxt[q];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < NP; q++) {
                        const int r = q * kWave + lane;
                        if (r < E) { slvl[r] = (uint16_t)bl[q]; mxb = max(mxb, (int)bl[q]); }
                    }
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) mxb = max(mxb, __shfl_xor(mxb, d));
                    wave_sync();
                } else {
                    for (int r = E - 1; r >= 0; r--) {
                        const uint8_t *arow = A + (size_t)perm[r] * W;
                        int mx = 0;
                        for (int base = r + 1; base < E; base += kWave) {
                            const int j = base + lane;
                            if (j < E && arow[j]) mx = max(mx, (int)slvl[j] + 1);
                        }
#pragma unroll
                        for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d));
                        if (lane == 0) slvl[r] = (uint16_t)mx;
                        mxb = max(mxb, mx);
                        wave_sync();
                    }
                }
            }
            if (lane == 0) { misc[12] = mxl; misc[13] = mxb; misc[14] = 0; }
        }
        __syncthreads();
        ML_STAMP(5);
        const int mxl = misc[12], mxb = misc[13];
        const int NL = mxl + 1 + (mxb + 1) + 1;
        const int lev_out = NL - 1;
        for (int t = tid; t < E; t += nthr) {
            const int w = perm[t];
            tslot[t] = (uint16_t)((w & 0x8000) ? nzr + atomicAdd(&misc[14], 1) : w);
        }
        for (int i = tid; i <= NL; i += nthr) hist[i] = 0u;
        __syncthreads();
        const int nslots = nzr + misc[14];
        // two passes over the same enumeration: pass 0 counts the ops of every level, pass 1 places them
        unsigned long long *ops = nullptr;
        bool emitted = true;
        for (int pass = 0; pass < 2 && emitted; pass++) {
            // level 0: known neighbours of every slot's check (stored rows at logical positions >= E are never read)
            for (int q = tid; q < nzr + E; q += nthr) {
                int sl_ = -1, chk = 0;
                if (q < nzr) { if ((int)iperm[q] < E) { sl_ = q; chk = orow[q]; } }
                else { const int w = perm[q - nzr]; if (w & 0x8000) { sl_ = tslot[q - nzr]; chk = w & 0x7FFF; } }
                if (sl_ < 0) continue;
                for (int tt = 0; tt < cd.degpad; tt++) {
                    const uint32_t col = cd.ell_col[(size_t)tt * mp + chk];
                    if (col == 0xFFFFu) break;
                    if (state[col]) continue;
                    if (pass == 0) atomicAdd(&hist[0], 1u);
                    else ops[atomicAdd(&hist[0], 1u)] = ml_op(kMlSlot0 + (uint32_t)sl_ * (uint32_t)a.solve_b, cd.ell_coef[(size_t)tt * mp + chk], col);
                }
            }
            // forward rows (wavefront per stored row) and backward rows (wavefront per logical row)
            for (int q = wave; q < nzr + (dont_do_jordan ? 0 : E); q += nw) {
                const bool fwd = q < nzr;
                int x, lo, hi, lev;
                if (fwd) {
                    x = q;
                    const int t = iperm[x];
                    if (t >= E || lvl[x] == 0u) continue;
                    lo = 0; hi = min(t, npiv); lev = (int)lvl[x];
                } else {
                    const int r = q - nzr;
                    x = perm[r]; lo = r + 1; hi = E; lev = mxl + 1 + (int)slvl[r];
                }
                const uint8_t *arow = A + (size_t)x * W;
                for (int base = lo; base < hi; base += kWave) {
                    const int j = base + lane;
                    const uint32_t b = (j < hi) ? (uint32_t)arow[j] : 0u;
                    const uint64_t mask = __ballot(b != 0u);
                    if (!mask) continue;
                    uint32_t pos = 0;
                    if (lane == 0) pos = atomicAdd(&hist[lev], (uint32_t)__popcll(mask));
                    pos = uniform(pos);
                    if (pass == 1 && b) {
                        const uint32_t cf = fwd ? b : (uint32_t)ex[(uint32_t)lg[b] + plog[j]];   // backward: a(r,j) / piv_j
                        ops[pos + __popcll(mask & ((1ull << lane) - 1ull))] =
                            ml_op(kMlSlot0 + (uint32_t)x * (uint32_t)a.solve_b, cf, kMlSlot0 + (uint32_t)perm[j] * (uint32_t)a.solve_b);
                    }
                }
            }
            // last level: the write-back
            for (int t = tid; t < E; t += nthr) {
                if (pass == 0) atomicAdd(&hist[lev_out], 1u);
                else ops[atomicAdd(&hist[lev_out], 1u)] = ml_op((uint32_t)elist[t], t < npiv ? ex[plog[t]] : 1u,
                                                                kMlSlot0 + (uint32_t)tslot[t] * (uint32_t)a.solve_b);
            }
            __syncthreads();
            ML_STAMP(6 + pass);
            if (pass == 0) {
                if (wave == 0) {   // counts -> start offsets; reserve the arena space
                    uint32_t carry = 0;
                    for (int base = 0; base < NL; base += kWave) {
                        const int idx = base + lane;
                        const uint32_t v = (idx < NL) ? hist[idx] : 0u;
                        uint32_t incl = v;
#pragma unroll
                        for (int d = 1; d < kWave; d <<= 1) {
                            const uint32_t t_ = __shfl_up(incl, d);
                            if (lane >= d) incl += t_;
                        }
                        if (idx < NL) hist[idx] = incl - v + carry;
                        carry += __shfl(incl, 63);
                    }
                    if (lane == 0) {
                        const unsigned long long need = (unsigned long long)carry + (unsigned long long)((NL + 2) / 2);
                        const unsigned long long off = atomicAdd(a.ops_head, need);
                        misc[15] = (off + need <= a.ops_cap) ? 1 : 0;
                        misc[22] = (int)(uint32_t)off; misc[23] = (int)(uint32_t)(off >> 32); misc[24] = (int)carry;
                    }
                }
                __syncthreads();
                emitted = misc[15] != 0;
                const unsigned long long off = (unsigned long long)(uint32_t)misc[22] | ((unsigned long long)(uint32_t)misc[23] << 32);
                ops = a.ops + off + (unsigned long long)((NL + 2) / 2);   // the level table sits in front of the ops
            }
        }
        if (emitted) {
            // hist[L] is now the END offset of level L: that is the level table
            uint32_t *tab = reinterpret_cast<uint32_t *>(ops - (unsigned long long)((NL + 2) / 2));
            for (int i = tid; i < NL; i += nthr) tab[i] = hist[i];
            if (tid == 0) {
                uint32_t *rec = a.rec + (size_t)slot * 8;
                rec[0] = (uint32_t)misc[22]; rec[1] = (uint32_t)misc[23]; rec[2] = (uint32_t)NL; rec[3] = (uint32_t)nslots;
                rec[4] = (uint32_t)misc[24]; rec[5] = 1u;
                rec[7] = a.mode == 3 ? 2u : 0u;   // 2: the second round of the solve kernel runs this schedule
                if (a.status) a.status[f] = dont_do_jordan ? LDPC_AMD_ST_ML_RANKDEF : LDPC_AMD_ST_ML_SOLVED;
            }
            return;
        }
        if (a.mode == 1) {   // no payload yet (the packet kernel is still running): the frame waits for the mode-2 launch
            if (tid == 0) { a.rec[(size_t)slot * 8 + 5] = 2u; atomicAdd(a.work + 1, 1); }
            return;
        }
        __syncthreads();
    }
    if (pk) {   // in-kernel solve (arena full, or LDPC_AMD_ML_SOLVE=0)
        if (tid == 0) {
            a.rec[(size_t)slot * 8 + 5] = 0u; a.rec[(size_t)slot * 8 + 7] = 0u;
            if (a.use_solve && a.mode == 0) atomicAdd(a.work + 1, 1);   // (statistics: a schedule that did not fit the arena)
        }
        build_packet_rhs();
        __syncthreads();
    }

    // ---- packets (in-kernel fall-back): forward solve in pull form.  Stored row x at logical position t collected the multipliers L[x][col],
    //      col < min(t, npiv); its right-hand side is final once the pivot rows of those columns are:
    //      R_x += sum L[x][col] R_{perm[col]}.  Rows are grouped by level (lvl[x], tracked during the factorisation); rows at
    //      logical positions >= E are never read or written back and are skipped.
    if (pk) {
        if (wave == 0) {
            int ns = 0, mxl = 0;
            for (int c0_ = 0; c0_ < nzr; c0_ += kWave) {
                const int c = c0_ + lane;
                const uint32_t L = (c < nzr && (int)iperm[c] < E) ? lvl[c] : 0u;
                const uint64_t mask = __ballot(L != 0u);
                if (L != 0u) {
                    const int pos = ns + __popcll(mask & ((1ull << lane) - 1ull));
                    steps[pos] = (uint32_t)c;
                    slvl[pos] = (uint16_t)L;
                }
                ns += __popcll(mask);
                mxl = max(mxl, (int)L);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) mxl = max(mxl, __shfl_xor(mxl, d));
            wave_sync();
            sort_steps_by_level(steps, slvl, ns, mxl, lvl, sorted);   // lvl[] now holds the level offsets
            if (lane == 0) misc[12] = mxl;
        }
        __syncthreads();
        ML_STAMP(8);
        const int mxl = misc[12];
        for (int L = 1; L <= mxl; L++) {
            const int s0 = (int)lvl[L - 1], s1 = (int)lvl[L];
            for (int s_ = s0 + wave; s_ < s1; s_ += nw) {
                const int x = (int)sorted[s_];
                const int lim = min((int)iperm[x], npiv);
                const uint8_t *arow = A + (size_t)x * W;
                uint8_t *rx = R + (size_t)x * a.Spad;
                for (int i0 = 0; i0 < rch; i0 += kWave) {
                    const int i = i0 + lane;
                    const bool act = i < rch;
                    U4 acc = {0, 0, 0, 0};
                    if (act) acc = *reinterpret_cast<const U4 *>(rx + i * 16);
                    for (int base = 0; base < lim; base += kWave) {
                        const uint32_t bL = (base + lane < lim) ? (uint32_t)arow[base + lane] : 0u;
                        uint64_t km = __ballot(bL != 0u);
                        while (km) {
                            U4 v[8];
                            uint32_t cf[8];
#pragma unroll
                            for (int u = 0; u < 8; u++) {
                                cf[u] = 0;
                                v[u] = U4{0, 0, 0, 0};
                                if (km) {
                                    const int e = __ffsll((long long)km) - 1;
                                    km &= km - 1;
                                    cf[u] = (uint32_t)__builtin_amdgcn_readlane((int)bL, e);
                                    const uint32_t src = perm[base + e];
                                    if (act) v[u] = *reinterpret_cast<const U4 *>(R + (size_t)src * a.Spad + i * 16);
                                }
                            }
#pragma unroll
                            for (int u = 0; u < 8; u++)
                                if (cf[u]) gfmac16(acc, load_multab(cf[u]), v[u]);
                        }
                    }
                    if (act) *reinterpret_cast<U4 *>(rx + i * 16) = acc;
                }
            }
            __syncthreads();
        }
    }
    ML_STAMP(9);

    // ---- Jordan elimination on the upper triangle, rhs only (:117-126).  Stored right-hand sides are unscaled:
    //      rhs_ref(r) = inv(piv_r) * R_r, so  rhs_ref(r) += A_ref(r,col) * rhs_ref(col)  <=>  R_r += a(r,col) * rhs_ref(col).
    if (!dont_do_jordan) {
        if (!PK) {
            // One wavefront, no barrier.  Lane l keeps the right-hand sides of the logical rows l, l + 64, ... in
            // registers (up to 8: E <= 512); column col's value is broadcast with v_readlane, so the only LDS round
            // trips on the dependent chain are log(value) and the antilog of the products; the U entries of the NEXT
            // column (and their logs) are fetched while the current column is applied.
            if (wave == 0 && E <= 512) {
                constexpr int NP = 8;
                uint32_t off[NP], rv[NP];
#pragma unroll
                for (int q = 0; q < NP; q++) {
                    const int r = q * kWave + lane;
                    off[q] = (r < E) ? (uint32_t)perm[r] * (uint32_t)W : 0u;
                    rv[q] = (r < E) ? (uint32_t)A[off[q] + ro] : 0u;
                }
                // lgu[q]: log of U(row, col) for the column about to be applied, 511 when the entry is zero or r >= col
                auto fetch_col = [&](int col, uint32_t (&lgu)[NP]) {
#pragma unroll
                    for (int q = 0; q < NP; q++) {
                        const int r = q * kWave + lane;
                        uint32_t v = 0;
                        if (q * kWave < col && r < col) v = A[off[q] + col];
                        lgu[q] = v ? (uint32_t)lg[v] : 511u;
                    }
                };
                uint32_t cur[NP], nxt[NP];
                fetch_col(E - 1, cur);
#pragma unroll
                for (int p = NP - 1; p >= 0; p--) {
                    if (p * kWave >= E) continue;
                    const int ltop = (E - 1 - p * kWave) < (kWave - 1) ? (E - 1 - p * kWave) : (kWave - 1);
                    for (int l = ltop; l >= 0; l--) {
                        const int col = p * kWave + l;
                        if (col == 0) break;
                        if (col > 1) fetch_col(col - 1, nxt);
                        const uint32_t rc = (uint32_t)__builtin_amdgcn_readlane((int)rv[p], l);
                        if (rc) {
                            const uint32_t lx = (uint32_t)lg[rc] + plog[col];
#pragma unroll
                            for (int q = 0; q <= p; q++)
                                if (cur[q] != 511u) rv[q] ^= ex[cur[q] + lx];
                        }
#pragma unroll
                        for (int q = 0; q < NP; q++) cur[q] = nxt[q];
                    }
                }
#pragma unroll
                for (int q = 0; q < NP; q++) {
                    const int r = q * kWave + lane;
                    if (r < E) A[off[q] + ro] = (uint8_t)rv[q];
                }
            } else if (wave == 0) {
                // E > 512: in place; the wavefront's LDS operations complete in order
                for (int col = E - 1; col >= 1; col--) {
                    const uint32_t rc = A[(size_t)perm[col] * W + ro];
                    if (rc) {
                        const uint32_t lx = (uint32_t)lg[rc] + plog[col];
                        for (int r = lane; r < col; r += kWave) {
                            uint8_t *row = A + (size_t)perm[r] * W;
                            const uint32_t v = row[col];
                            if (v) row[ro] ^= ex[(uint32_t)lg[v] + lx];
                        }
                    }
                    wave_sync();
                }
            }
            __syncthreads();
        } else {
            // Packets, pull form: X_r = inv(piv_r) (R_{perm[r]} + sum_{j > r, a(r,j) != 0} a(r,j) X_j), the solved symbols X
            // being read from (and written to) `out`.  Level of row r = 1 + max level of the rows j it reads; one wavefront
            // walks the rows from the last to the first to find the levels (a row's entries sit in its matrix row).
            if (wave == 0) {
                int mxb = 0;
                for (int r = E - 1; r >= 0; r--) {
                    const uint8_t *arow = A + (size_t)perm[r] * W;
                    int mx = 0;
                    for (int base = r + 1; base < E; base += kWave) {
                        const int j = base + lane;
                        if (j < E && arow[j]) mx = max(mx, (int)slvl[j] + 1);
                    }
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d));
                    if (lane == 0) { slvl[r] = (uint16_t)mx; steps[r] = (uint32_t)r; }
                    mxb = max(mxb, mx);
                    wave_sync();
                }
                sort_steps_by_level(steps, slvl, E, mxb, lvl, sorted);
                if (lane == 0) misc[13] = mxb;
            }
            __syncthreads();
            ML_STAMP(10);
            const int mxb = misc[13];
            for (int L = 0; L <= mxb; L++) {
                const int s0 = L ? (int)lvl[L - 1] : 0, s1 = (int)lvl[L];
                for (int s_ = s0 + wave; s_ < s1; s_ += nw) {
                    const int r = (int)sorted[s_];
                    const int x = perm[r];
                    const uint8_t *arow = A + (size_t)x * W;
                    const uint8_t *rx = R + (size_t)x * a.Spad;
                    uint8_t *dst = fout + (int64_t)elist[r] * S;
                    const MulTab ts = load_multab(uniform(ex[plog[r]]));   // inv(pivot of row r)
                    for (int i0 = 0; i0 < rch; i0 += kWave) {
                        const int i = i0 + lane;
                        const bool act = i < rch;
                        U4 acc = {0, 0, 0, 0};
                        if (act) acc = *reinterpret_cast<const U4 *>(rx + i * 16);
                        for (int base = r + 1; base < E; base += kWave) {
                            const uint32_t bU = (base + lane < E) ? (uint32_t)arow[base + lane] : 0u;
                            uint64_t km = __ballot(bU != 0u);
                            while (km) {
                                U4 v[8];
                                uint32_t cf[8];
#pragma unroll
                                for (int u = 0; u < 8; u++) {
                                    cf[u] = 0;
                                    v[u] = U4{0, 0, 0, 0};
                                    if (km) {
                                        const int e = __ffsll((long long)km) - 1;
                                        km &= km - 1;
                                        cf[u] = (uint32_t)__builtin_amdgcn_readlane((int)bU, e);
                                        const uint32_t sc = elist[base + e];
                                        if (act) v[u] = row_load16<W4>(fout + (int64_t)sc * S + fo(i));
                                    }
                                }
#pragma unroll
                                for (int u = 0; u < 8; u++)
                                    if (cf[u]) gfmac16(acc, load_multab(cf[u]), v[u]);
                            }
                        }
                        if (act) row_store16<W4>(dst + fo(i), gfmul16(ts, acc));
                    }
                }
                __syncthreads();
            }
        }
    }

    // ---- y_current(erasure_ind) = rhs(1:E) -- unconditional (:127).  Logical row t: a pivot row (t < brk, or every
    //      row when the elimination completed) carries the scale the reference applied at :99-105.
    ML_STAMP(11);
    if (!PK) {
        for (int t = tid; t < E; t += nthr) {
            const int w = perm[t];
            uint32_t v;
            if (w & 0x8000) v = ml_rhs_byte(cd, nullptr, state, fout, lg, ex, w & 0x7FFF);
            else v = A[(size_t)w * W + ro];
            if (t < npiv && v) v = ex[(uint32_t)lg[v] + plog[t]];
            fout[elist[t]] = (uint8_t)v;   // only erased positions are written; ml_rhs_byte reads known symbols only
        }
    } else if (dont_do_jordan) {   // (a full-rank packet frame was written by the backward solve above)
        for (int t = wave; t < E; t += nw) {
            const int w = perm[t];
            uint8_t *dst = fout + (int64_t)elist[t] * S;
            if (w & 0x8000) {   // all-zero row of a rank-deficient frame: its right-hand side was never needed until now
                const int r = w & 0x7FFF;
                for (int i = lane; i < rch; i += kWave) {
                    U4 acc = {0, 0, 0, 0};
                    for (int tt = 0; tt < cd.degpad; tt++) {
                        const uint32_t col = cd.ell_col[(size_t)tt * mp + r];
                        if (col == 0xFFFFu) break;
                        if (state[col]) continue;
                        const U4 v = row_load16<W4>(fout + (int64_t)col * S + fo(i));
                        gfmac16(acc, load_multab(uniform(cd.ell_coef[(size_t)tt * mp + r])), v);
                    }
                    row_store16<W4>(dst + fo(i), acc);
                }
            } else {
                const uint8_t *src = R + (size_t)w * a.Spad;
                const MulTab ts = load_multab(uniform(t < npiv ? ex[plog[t]] : 1u));
                for (int i = lane; i < rch; i += kWave)
                    row_store16<W4>(dst + fo(i), gfmul16(ts, *reinterpret_cast<const U4 *>(src + i * 16)));
            }
        }
    }
    ML_STAMP(12);
    if (tid == 0 && a.status) a.status[f] = dont_do_jordan ? LDPC_AMD_ST_ML_RANKDEF : LDPC_AMD_ST_ML_SOLVED;
}

template <bool W4>
__device__ __forceinline__ void ml_kernel_body(const MlArgs &a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const DevCode &cd = a.code;
    const int n = cd.n, m = cd.m;
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int lane = lane_id(), wave = wave_id();

    uint16_t *colmap = reinterpret_cast<uint16_t *>(smem + a.lds_colmap);
    uint16_t *elist = reinterpret_cast<uint16_t *>(smem + a.lds_elist);
    uint16_t *perm = reinterpret_cast<uint16_t *>(smem + a.lds_perm);
    uint16_t *iperm = reinterpret_cast<uint16_t *>(smem + a.lds_iperm);
    uint16_t *orow = reinterpret_cast<uint16_t *>(smem + a.lds_orow);
    uint32_t *mt = reinterpret_cast<uint32_t *>(smem + a.lds_mt);
    uint8_t *lg = smem + a.lds_lg, *ex = smem + a.lds_ex;
    int *misc = reinterpret_cast<int *>(smem + a.lds_misc);   // [0] E  [1] nzr  [2] slot  [4..6] cnt  [8..10] pcbuf ; +64: key[3]
    uint32_t *key = reinterpret_cast<uint32_t *>(smem + a.lds_misc + 64);

    // The residual count is final when this kernel starts (the peel kernel precedes it on the stream): a batch message passing
    // completed -- every batch at 10 % erasures -- costs the launch and one scalar load, not the table staging of every workgroup.
    const int count = a.ml_list[0];
    if (count == 0) return;
    if (a.mode == 2 && a.work[1] == 0) return;   // nothing was deferred
    if (a.mode == 3 && *a.nfail == 0) return;    // every fast-path solution passed its check
    int32_t *handout = a.mode == 2 ? a.work2 : (a.mode == 3 ? a.work3 : a.work);
    for (int i = tid; i < 2048; i += nthr) mt[i] = c_mul3[(uint32_t)c_exp[i >> 3] * 8 + (i & 7)];   // row l = table of alpha^l
    for (int i = tid; i < 256; i += nthr) lg[i] = c_log[i];
    for (int i = tid; i < 1024; i += nthr) ex[i] = c_exp[i % 255];
    int *cls = misc + 32;                                     // counts of the size classes
    if (tid < kMlClasses) cls[tid] = a.ml_list[1 + tid];

    for (;;) {
        __syncthreads();
        if (tid == 0) {   // work items walk the size classes, largest systems first
            const int item = atomicAdd(handout, 1);
            int sl_ = -1;
            if (item < count) {
                int i = item, k_ = 0;
                while (k_ < kMlClasses - 1 && i >= cls[k_]) { i -= cls[k_]; k_++; }
                sl_ = a.ml_list[kMlHdr + a.nframes + (int64_t)k_ * a.nframes + i];
            }
            misc[2] = item; misc[3] = sl_;
        }
        __syncthreads();
        if (misc[2] >= count) break;
        const int slot = misc[3];
        if (a.mode == 2) { if (a.rec[(size_t)slot * 8 + 5] != 2u) continue; }   // only the deferred frames
        else if (a.mode == 3) { if (!a.rec[(size_t)slot * 8 + 6] || a.rec[(size_t)slot * 8 + 7] != 1u) continue; }   // only the flagged ones
        else if (a.use_pi && a.rec[(size_t)slot * 8 + 6]) continue;   // the fast path emitted this frame's schedule (full rank: same bytes)
        const int64_t f = a.ml_list[kMlHdr + slot];
        const uint8_t *state = a.ml_state + (int64_t)slot * n;

        // ---- erasure_ind = find(y_current == -1), ascending (:63)
        if (wave == 0) {
            int E = 0;
            for (int j0 = 0; j0 < n; j0 += kWave) {
                const int j = j0 + lane;
                const bool e = (j < n) && state[j];
                const uint64_t mask = __ballot(e);
                const int pos = E + __popcll(mask & ((1ull << lane) - 1ull));
                if (j < n) colmap[j] = e ? (uint16_t)pos : (uint16_t)0xFFFFu;
                if (e) elist[pos] = (uint16_t)j;
                E += __popcll(mask);
            }
            if (lane == 0) {
                misc[0] = E; misc[1] = 0;
                misc[4] = misc[5] = misc[6] = 0;
                key[0] = key[1] = key[2] = kMlNoPivot;
            }
        }
        __syncthreads();
        const int E = misc[0];
        // ---- the rows of H(:, erased) that are not all-zero get a stored row; perm starts as the identity (:65)
        for (int r0 = wave * kWave; r0 < m; r0 += nthr) {
            const int r = r0 + lane;
            bool nz = false;
            if (r < m) {
                for (int t = 0; t < cd.degpad && !nz; t++) {
                    const uint32_t col = cd.ell_col[(size_t)t * cd.mpad + r];
                    if (col == 0xFFFFu) break;
                    nz = colmap[col] != 0xFFFFu;
                }
            }
            const uint64_t mask = __ballot(nz);
            int base = 0;
            if (lane == 0 && mask) base = atomicAdd(&misc[1], __popcll(mask));
            base = __shfl(base, 0);
            if (r < m) {
                if (nz) {
                    const int c = base + __popcll(mask & ((1ull << lane) - 1ull));
                    perm[r] = (uint16_t)c; orow[c] = (uint16_t)r; iperm[c] = (uint16_t)r;
                } else {
                    perm[r] = (uint16_t)(0x8000 | r);
                }
            }
        }
        __syncthreads();
        const int nzr = misc[1];
        if (tid == 0) misc[8] = perm[0];
        const int ach = (E + 15) >> 4;                        // 16-byte chunks of the matrix part
        const int nch = (ach + (a.S == 1 ? 1 : 0)) | 1;      // + the rhs chunk when S == 1; odd (LDS banks)
        const bool in_lds = nzr * (nch << 4) <= a.capA;
        if (a.S == 1) {
            if (in_lds) ml_frame<true, false>(a, f, slot, state, E, nzr, nch, ach);
            else ml_frame<false, false>(a, f, slot, state, E, nzr, nch, ach);
        } else {
            if (in_lds) ml_frame<true, true, W4>(a, f, slot, state, E, nzr, nch, ach);
            else ml_frame<false, true, W4>(a, f, slot, state, E, nzr, nch, ach);
        }
    }
}

__global__ __launch_bounds__(1024) void ldpc_ml_kernel(MlArgs a) { ml_kernel_body<false>(a); }
// the word form (S a multiple of 4, not of 16: ml_frame<..., W4>); never launched for S = 1
__global__ __launch_bounds__(1024) void ldpc_ml_words_kernel(MlArgs a) { ml_kernel_body<true>(a); }

// =================================================================================================
// Packets: executes the solve schedules the ML kernel emitted.  One workgroup per (ML frame, B-byte slice of its rows);
// every stored row has a B-byte slot in LDS; ops "slot[dst] ^= coef * source" run level by level with one workgroup barrier
// per level -- an LDS round trip per level instead of an L2 round trip per column.  Ops are dealt round-robin to the lane
// groups (LPR lanes x 16 bytes = one slot); level 0 (the known neighbours, read from `out` in HBM) keeps eight rows in
// flight per lane group, the first op of a later level is requested three levels ahead.
// =================================================================================================
struct MlSolveArgs {
    DevCode code;
    int S, nslices;
    int piece_last;           // S - B: piece sl of a row starts at min(sl * B, piece_last) (the word form's last piece overlaps its neighbour)
    int64_t nframes;          // frames of the batch (stride of the size-class lists)
    const int32_t *ml_list;
    uint32_t *rec;           // [7]: set to 1 by the first workgroup that finds a non-zero check of a fast-path schedule
    const unsigned long long *ops;
    uint8_t *out;
    int32_t *work;           // task hand-out counter
    int32_t *nfail;          // frames flagged that way
    int round;               // 1: every emitted schedule.  2: the schedules the exact kernel emitted for the flagged frames (rec[7] = 2)
    int lds_tab, lds_mt, lds_misc;   // byte offsets behind the slots
    int *err;                        // pinned host word: device-error bits (kDevErrLdsBase)
    int dbg;                         // diagnostic build only (-DLDPC_AMD_MLDBG, tools/sens_ml.py)
};

// W4 (ldpc_ml_solve_words_kernel): S is a multiple of 4, not of 16 -- ceil(S / B) pieces, the last one moved back to end with the
// row, 4-byte accesses.  The overlap is safe: level 0 READS known rows (received, or solved by the packet kernel: an earlier launch),
// the last level WRITES unknown rows -- disjoint sets -- and everything in between lives in this workgroup's LDS slots; the two pieces
// that share bytes write the same values there.
template <int LPR, bool W4>
__device__ __forceinline__ void ml_solve_body(const MlSolveArgs &a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int B = 16 * LPR;
    const int n = a.code.n, S = a.S;
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int lane = lane_id();
    const int g = tid / LPR, gl = tid % LPR, NG = nthr / LPR, h = (lane >> 3) & 1;
    // LDS: [0, 8192) multiply tables | [kMlSlot0, ...) the slots | level table | misc -- the op words carry LDS addresses
    typedef __attribute__((address_space(3))) unsigned char lds_u8;
    // (no static __shared__ may be declared in this kernel: the op words carry absolute LDS addresses; a violation is reported
    // through the context's device-error word -> LDPC_AMD_EHIP at the next synchronising call, never a silent wrong answer)
    if ((uint32_t)(uintptr_t)(lds_u8 *)(smem) != 0u) {
        if (threadIdx.x == 0 && a.err) atomicOr(a.err, kDevErrLdsBase);
        return;
    }
    unsigned char *slots = smem + kMlSlot0;
    uint32_t *ltab = reinterpret_cast<uint32_t *>(smem + a.lds_tab);
    uint32_t *mt = reinterpret_cast<uint32_t *>(smem);
    int *misc = reinterpret_cast<int *>(smem + a.lds_misc);
    const int count = a.ml_list[0];
    if (count == 0) return;   // nothing reached the ML stage: no table staging either
    if (a.round == 2 && *a.nfail == 0) return;
    for (int i = tid; i < 2048; i += nthr) mt[i] = c_mul3[i];
    const int ntasks = count * a.nslices;
    int *cls = misc + 4;                                      // counts of the size classes
    if (tid < kMlClasses) cls[tid] = a.ml_list[1 + tid];
#ifdef LDPC_AMD_STAMPS
    unsigned long long sv_prev = __builtin_amdgcn_s_memtime();
#define SV_STAMP(i) do { if (tid == 0) { const unsigned long long t__ = __builtin_amdgcn_s_memtime(); atomicAdd(&g_peel_stamps[32 + (i)], t__ - sv_prev); sv_prev = t__; } } while (0)
#else
#define SV_STAMP(i) do { } while (0)
#endif
    for (;;) {
        __syncthreads();
        SV_STAMP(4);   // output level + wait for the slowest wavefront
        if (tid == 0) {   // tasks walk the size classes like the ML kernel: the slices of the largest systems first
            const int task = atomicAdd(a.work, 1);
            int sl_ = -1;
            if (task < ntasks) {
                int i = task / a.nslices, k_ = 0;
                while (k_ < kMlClasses - 1 && i >= cls[k_]) { i -= cls[k_]; k_++; }
                sl_ = a.ml_list[kMlHdr + a.nframes + (int64_t)k_ * a.nframes + i];
            }
            misc[0] = task; misc[1] = sl_;
        }
        __syncthreads();
        const int task = misc[0];
        if (task >= ntasks) break;
        const int slot = misc[1];
        const int sl = task % a.nslices;
        uint32_t *rec = a.rec + (size_t)slot * 8;
        if (!rec[5]) continue;   // this frame was solved inside the ML kernel
        if (a.round == 2 && rec[7] != 2u) continue;
        const unsigned long long off = (unsigned long long)rec[0] | ((unsigned long long)rec[1] << 32);
        const int NL = (int)rec[2], nslots = (int)rec[3];
        const uint32_t total = rec[4];
        const uint32_t *tab = reinterpret_cast<const uint32_t *>(a.ops + off);
        const unsigned long long *ops = a.ops + off + (unsigned long long)((NL + 2) / 2);
        const int64_t f = a.ml_list[kMlHdr + slot];
        uint8_t *fout = a.out + f * (int64_t)n * S + (int64_t)(W4 ? min(sl * B, a.piece_last) : sl * B) + gl * 16;
        for (int i = tid; i < NL; i += nthr) ltab[i] = tab[i];
        for (int i = tid; i < nslots * LPR; i += nthr) reinterpret_cast<U4 *>(slots)[i] = U4{0, 0, 0, 0};
        // Ops of a level are dealt round-robin to the lane groups, restarting at every level: group g takes ops o0 + g,
        // o0 + g + NG, ...  All loads of the pipelined parts are UNCONDITIONAL (indices clamped into the stream; any op word
        // yields a valid row address) and live in registers with static indices, so that the hardware counter, not a
        // wait-for-everything, orders them.
        auto opat = [&](uint32_t idx) { return ops[idx < total ? idx : total - 1u]; };
        const uint32_t lane_a = (uint32_t)(gl * 16 + h * 8), lane_b = (uint32_t)(gl * 16 + (1 - h) * 8), lane_16 = (uint32_t)(gl * 16);
        auto execute = [&](unsigned long long op, const U4 &srcv) {
            const uint32_t lo = (uint32_t)op;
            const U4 prod = gfmul16(lds_multab_at(lo >> 19), srcv);
            lds_xor16_at((lo & 0x00FFFFFFu) | lane_a, (lo & 0x007FFFFFu) | lane_b, prod, h);
        };
        auto slot_of = [&](unsigned long long op) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
            const u32x4 q = *reinterpret_cast<const lds_u32x4 *>((uintptr_t)((uint32_t)(op >> 32) | lane_16));
            return U4{q.x, q.y, q.z, q.w};
        };
        const uint32_t nm1 = (uint32_t)n - 1u;
        auto row_of = [&](uint32_t sym) { return fout + (int64_t)min(sym & 0xFFFFu, nm1) * S; };   // (clamped: prefetched op words of later levels are not symbols)
        __syncthreads();
        SV_STAMP(0);   // task pick-up, level table, slot zeroing
        const uint32_t e0 = ltab[0];
        // ---- level 0: slot[dst] ^= h * out[symbol].  C rows in flight per lane group; the op words of the next chunk are
        //      requested behind the rows of this one.
        {
            constexpr int C = 8;
            unsigned long long oq[C], on[C];
            U4 vr[C];
#pragma unroll
            for (int i = 0; i < C; i++) oq[i] = opat((uint32_t)g + (uint32_t)i * NG);
#ifdef LDPC_AMD_MLDBG
            const uint32_t e0x = (a.dbg & 16384) ? 0u : e0;   // level 0 skipped (WRONG bytes): what the known-row re-read and its products cost
#else
            const uint32_t e0x = e0;
#endif
            for (uint32_t base = (uint32_t)g; base < e0x; base += (uint32_t)(C * NG)) {
#pragma unroll
                for (int i = 0; i < C; i++) vr[i] = row_load16<W4>(row_of((uint32_t)(oq[i] >> 32)));
#pragma unroll
                for (int i = 0; i < C; i++) on[i] = opat(base + (uint32_t)((C + i) * NG));
#pragma unroll
                for (int i = 0; i < C; i++)
                    if (base + (uint32_t)(i * NG) < e0) execute(oq[i], vr[i]);
#ifdef LDPC_AMD_MLDBG
                if (a.dbg & 512) {   // the multiply-accumulates of level 0 twice (the second time cancels the first: XOR)
#pragma unroll
                    for (int i = 0; i < C; i++)
                        if (base + (uint32_t)(i * NG) < e0) { execute(oq[i], vr[i]); execute(oq[i], vr[i]); }
                }
#endif
#pragma unroll
                for (int i = 0; i < C; i++) oq[i] = on[i];
            }
        }
        __syncthreads();
        SV_STAMP(1);   // level 0
        // ---- forward and backward levels: slot[dst] ^= coef * slot[src].  The first op of a level is requested three
        //      levels ahead (three registers, used in turn); the few levels with more ops than lane groups fetch the rest on
        //      demand (batched or run-wise fetching of those was measured slower: DESIGN.md).
        {
            constexpr int PF = 3;
            unsigned long long p[PF];
            auto level_start = [&](int L) { return L <= 0 ? 0u : ltab[L - 1 < NL ? L - 1 : NL - 1]; };
#pragma unroll
            for (int u = 0; u < PF; u++) p[u] = opat(level_start(1 + u) + (uint32_t)g);
#ifdef LDPC_AMD_MLDBG
            if (a.dbg & 256) {   // every forward / backward op as ONE level (WRONG bytes): the most any composition of levels could reach
                const uint32_t oA = ltab[0], oB = NL >= 2 ? ltab[NL - 2] : ltab[0];
                for (uint32_t idx = oA + (uint32_t)g; idx < oB; idx += (uint32_t)NG) {
                    const unsigned long long o2 = ops[idx];
                    execute(o2, slot_of(o2));
                }
                __syncthreads();
            } else
#endif
            for (int L = 1; L + 1 < NL; L += PF) {
#pragma unroll
                for (int u = 0; u < PF; u++) {
                    const int Lu = L + u;
                    if (Lu + 1 < NL) {
                        const uint32_t o0 = ltab[Lu - 1], o1 = ltab[Lu];
                        const unsigned long long op = p[u];
                        p[u] = opat(level_start(Lu + PF) + (uint32_t)g);
                        uint32_t idx = o0 + (uint32_t)g;
                        if (idx < o1) execute(op, slot_of(op));
                        for (idx += (uint32_t)NG; idx < o1; idx += (uint32_t)NG) {
                            const unsigned long long o2 = ops[idx];
                            execute(o2, slot_of(o2));
#ifdef LDPC_AMD_MLDBG
                            if (a.dbg & 1024) { execute(o2, slot_of(o2)); execute(o2, slot_of(o2)); }   // twice more: cancels
#endif
                        }
#ifdef LDPC_AMD_MLDBG
                        if ((a.dbg & 1024) && o0 + (uint32_t)g < o1) { execute(op, slot_of(op)); execute(op, slot_of(op)); }
                        if (a.dbg & 2048) __syncthreads();
                        if ((a.dbg & 4096) && (Lu & 1)) continue;   // no barrier behind the odd levels (WRONG bytes): what halving the level count would buy
                        if ((a.dbg & 8192) && (Lu & 3)) continue;   // ... a barrier behind every fourth level only: a quarter of the levels
#endif
                        __syncthreads();
                    }
                }
            }
        }
        SV_STAMP(2);   // forward + backward levels
        // ---- last level: out[symbol] = scale * slot[src]
        {
            constexpr int C = 4;
            for (uint32_t base = (NL >= 2 ? ltab[NL - 2] : 0u) + (uint32_t)g; base < total; base += (uint32_t)(C * NG)) {
                unsigned long long oq[C];
#pragma unroll
                for (int i = 0; i < C; i++) oq[i] = opat(base + (uint32_t)(i * NG));
#pragma unroll
                for (int i = 0; i < C; i++)
                    if (base + (uint32_t)(i * NG) < total) {
                        const U4 val = slot_of(oq[i]);
                        if (((uint32_t)oq[i] & 0xFFFFu) == 0xFFFFu) {   // a check op of the fast path: an equation it did not use must hold
                            if ((val.x | val.y | val.z | val.w) != 0u && atomicExch(&rec[7], 1u) == 0u) atomicAdd(a.nfail, 1);
                        } else {
                            row_store16<W4>(row_of((uint32_t)oq[i]), gfmul16(lds_multab_at((uint32_t)oq[i] >> 19), val));
                        }
                    }
            }
        }
    }
}

template <int LPR>
__global__ __launch_bounds__(512, 4) void ldpc_ml_solve_kernel(MlSolveArgs a) { ml_solve_body<LPR, false>(a); }
template <int LPR>
__global__ __launch_bounds__(512, 4) void ldpc_ml_solve_words_kernel(MlSolveArgs a) { ml_solve_body<LPR, true>(a); }
