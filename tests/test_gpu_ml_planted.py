"""The ML stage (csrc/ml_kernel.inc, csrc/ml_pi.inc, the solve kernel) on PLANTED residual systems, GPU, through the C-ABI.

The other suites reach the GPU elimination with what the built-in and random codes happen to leave.  Here the residual system
is chosen (tools/ml_plant.py; tests/test_ml_planted_cpu.py asserts that every case has the property it was designed for): pivots
hundreds of rows below the diagonal in every column, all-zero rows in the first E logical positions of rank-deficient frames
that are not codewords, E on either side of every multiple of 16 up to 64 and at 150 and 300, E = m and E = m + 1, breaks at the
second, a middle and the last column, fewer and twice as many touched checks as unknowns, blocks no peeling gets through.
Codes (600,300), (2048,1024), and (8192,4096) planted in rows >= 4000: 4096 checks is the ML stage's limit (plan_ml; launch_decode
answers LDPC_AMD_EUNSUP above it: the pivot key has 12-bit row fields), and registration and decode accept it.

The library registers rows of up to 24 entries, so a block with ALL entries non-zero ends at E = 20 here (E = 64 is on the CPU
side, oracle against the literal model); `band` -- 16 cyclic diagonals, 15 inactivations -- is the dense family up to E = 300.

EVERY frame of every batch is compared with the oracle (Matlab/My_LDPC_HybridML_NonBinary_Erasure_Decoder.m:13-129): bytes,
sweeps, residual, status.  Status 3 (more unknowns than checks, the reference stops with an error): received symbols unchanged,
sweep-solved symbols the oracle's.  Every knob set must equal the default run bit for bit.  ml_stats() says which path ran."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ml_plant as mp  # noqa: E402
from pi_model import INV, MUL  # noqa: E402

from ldpc_erasure_codes_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(mp.CASES)
WHAT = ("out", "sweeps", "residual", "status")
KNOB_NAMES = ("ML_PI", "ML_OVERLAP", "ML_SOLVE", "ML_SOLVE_B", "ML_PACK", "ML_THREADS", "ML_ARENA_WORDS", "ML_PI_IMAX")
# packets; each equals the default run bit for bit
KNOB_SETS = [{"ML_PI": "0"}, {"ML_PI": "1"}, {"ML_OVERLAP": "0"}, {"ML_OVERLAP": "1"}, {"ML_OVERLAP": "2"}, {"ML_SOLVE": "0"},
             {"ML_SOLVE": "1"}, {"ML_SOLVE_B": "16"}, {"ML_SOLVE_B": "128"}, {"ML_PACK": "1"}, {"ML_PACK": "4"},
             {"ML_THREADS": "256"}, {"ML_THREADS": "1024"}, {"ML_ARENA_WORDS": "1024"},
             {"ML_PI": "0", "ML_PACK": "4"}, {"ML_PI": "0", "ML_SOLVE": "0", "ML_PACK": "4"}, {"ML_PI": "0", "ML_ARENA_WORDS": "1024", "ML_OVERLAP": "1"}]
KNOB_SETS_S1 = [{"ML_PACK": "1"}, {"ML_PACK": "4"}, {"ML_THREADS": "256"}, {"ML_THREADS": "1024"}, {"ML_PACK": "4", "ML_THREADS": "256"}]
# S = 1024 (eight 128-byte slices per row in the solve kernel) on these
S1024 = ("n600_anti_E33_bottom", "n600_band_E64_top", "n600_dupcol32_E64_bottom", "n600_tall_E33_T66_clusters", "n600_wide_E64_T50_bottom",
         "n600_circulant2_singular_E17_clusters", "n600_generic_singular_E64_top", "n600_generic_tall_E33_T66_top", "n2048_anti_E64_bottom", "n8192_dupcol24_E48_bottom", "n100_band_E40_top")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    # a packet batch WITHOUT a frame for the ML stage (the E = m + 1 case: every frame is all clear or has more unknowns than checks)
    # makes the next batch skip the fast path (ML_PI_ADAPTIVE, tests/test_gpu_ml_fast_path.py): same bytes, but the counts asserted
    # here would depend on the order of the tests
    c.configure("LDPC_AMD_ML_PI_ADAPTIVE", "0")
    yield c
    c.close()


def _configure(ctx, knobs):
    for k in KNOB_NAMES:
        ctx.configure("LDPC_AMD_" + k, knobs.get(k))


def _oracle_frames(oc, sym, era, S):
    """Per frame: (bytes [n, S], symbols still unknown [n], iterations, residual count, status word)."""
    exp = []
    for f in range(sym.shape[0]):
        o_out, o_unk, o_it, info, rc = oc.decode_packets(sym[f].reshape(oc.n, S), era[f])
        want = 0 if info[0] == 0 else (3 if (rc == -2 or not info[1]) else (2 if info[2] else 1))
        exp.append((o_out, o_unk.astype(bool), o_it, int(info[0]), want))
    return exp


def _equals_the_oracle(got, exp, sym, era, S, what):
    out, sw, res, st = got
    n = sym.shape[1]
    for f, (o_out, o_unk, o_it, o_res, want) in enumerate(exp):
        ctxt = what + (f,)
        assert (int(sw[f]), int(res[f]), int(st[f])) == (o_it, o_res, want), (ctxt, sw[f], o_it, res[f], o_res, st[f], want)
        g = out[f].reshape(n, S)
        if want != 3:
            assert np.array_equal(g, o_out), ctxt
        else:   # ML not run: what was received stays as it is, what the sweeps solved is the oracle's
            known = era[f] == 0
            solved = ~known & ~o_unk
            assert np.array_equal(g[known], sym[f].reshape(n, S)[known]), ctxt
            assert np.array_equal(g[solved], o_out[solved]), ctxt


def _same(a, b, what):
    for x, y, w in zip(a, b, WHAT):
        assert np.array_equal(x, y), (what, w)


def _max_col_degree(code):
    return int(np.bincount(code.cols.astype(np.int64), minlength=code.n).max())


def _inconsistent(code, sym, era):
    """True when the residual system H(touched, erased) x = rhs of a frame whose sweeps solve nothing has NO solution in some byte
    lane (rank [A | rhs] > rank A): what the verified fast path must flag.  sym [n, S]."""
    unk = era.astype(bool)
    cols = np.flatnonzero(unk)
    pos = np.full(code.n, -1, dtype=np.int64)
    pos[cols] = np.arange(cols.size)
    rp = code.row_ptr.astype(np.int64)
    A, R = [], []
    for r in range(code.m):
        c, h = code.cols[rp[r]:rp[r + 1]].astype(np.int64), code.coefs[rp[r]:rp[r + 1]]
        if not unk[c].any():
            continue
        a = np.zeros(cols.size, dtype=np.uint8)
        a[pos[c[unk[c]]]] = h[unk[c]]
        b = np.zeros(sym.shape[1], dtype=np.uint8)
        for j, hj in zip(c[~unk[c]], h[~unk[c]]):
            b ^= MUL[int(hj)][sym[j]]
        A.append(a)
        R.append(b)
    M = np.concatenate([np.stack(A), np.stack(R)], axis=1)
    E, r = cols.size, 0
    for c in range(E):
        piv = np.flatnonzero(M[r:, c])
        if piv.size == 0:
            continue
        p = r + int(piv[0])
        M[[r, p]] = M[[p, r]]
        M[r] = MUL[int(INV[M[r, c]])][M[r]]
        rows = np.flatnonzero(M[:, c])
        rows = rows[rows != r]
        M[rows] ^= MUL[M[rows, c][:, None], M[r][None, :]]
        r += 1
        if r == M.shape[0]:
            break
    return bool(M[r:, E:].any())


def _shape(sym, S):
    return np.ascontiguousarray(sym[:, :, 0] if S == 1 else sym)


def matrix_bytes(T, E, S):
    """Bytes of a stored residual system: T non-zero rows of 16 * (odd number of chunks), the chunks of E unknowns + at S = 1 one
    more for the right-hand side (csrc/ml_kernel.inc, "Storage")."""
    return T * 16 * ((((E + 15) // 16) + (1 if S == 1 else 0)) | 1)


@pytest.mark.parametrize("name", CASES)
def test_planted_case_equals_the_oracle_under_every_knob_set(ctx, oracle, name):
    c = mp.CASES[name]
    code = mp.case_code(name)
    oc = oracle.OracleCode(code)
    m = code.m
    pr = mp.properties(code, mp.erasures(code))
    h = ctx.register_code(code)
    fast_path = _max_col_degree(code) <= mp.DEVICE_COL_DEG      # longer columns: the code has no fast path, everything is exact
    seed = 1000 + CASES.index(name)
    try:
        for S in (1, 16, 64) + ((1024,) if name in S1024 else ()):
            sym, era, kinds = mp.case_frames(oc, code, pr, S, seed + S)
            exp = _oracle_frames(oc, sym, era, S)
            want_st = np.array([e[4] for e in exp])
            assert want_st[kinds.index("codeword")] == pr["status"] and want_st[-1] == 0, (name, want_st)
            x = _shape(sym, S)
            _configure(ctx, {})
            ref = ctx.decode(h, x, era)
            ms = ctx.ml_stats()
            _equals_the_oracle(ref, exp, sym, era, S, (name, S, "default"))
            n_res = int(sum(1 for e in exp if 0 < e[3] <= m))
            assert ms["residual_frames"] == n_res, (name, S, ms)
            if S == 1:
                for knobs in KNOB_SETS_S1:
                    _configure(ctx, knobs)
                    _same(ctx.decode(h, x, era), ref, (name, S, knobs))
                continue
            # which path: flagged = the status-1 frames whose system the corruption made inconsistent (a square full-rank block
            # stays consistent whatever the right-hand side: only surplus checks can contradict), all through the fast path
            n_bad = sum(1 for f, k in enumerate(kinds) if k == "touched" and want_st[f] == 1 and _inconsistent(code, sym[f], era[f]))
            if c["kind"] in ("tall", "generic_tall"):
                assert n_bad == 1, (name, S)
            if fast_path:
                assert 0.8 * n_bad <= ms["flagged_frames"] <= n_bad, (name, S, ms, n_bad)
                assert ms["fast_path_frames"] == int((want_st == 1).sum()), (name, S, ms)
            else:
                assert ms["fast_path_frames"] == 0 and ms["flagged_frames"] == 0, (name, S, ms)
            for knobs in KNOB_SETS:
                _configure(ctx, knobs)
                _same(ctx.decode(h, x, era), ref, (name, S, knobs))
                ms = ctx.ml_stats()
                assert ms["residual_frames"] == n_res, (name, S, knobs, ms)
                if knobs.get("ML_PI") == "0" or knobs.get("ML_SOLVE") == "0":
                    assert ms["fast_path_frames"] == 0 and ms["flagged_frames"] == 0, (name, S, knobs, ms)
                if "ML_ARENA_WORDS" in knobs and knobs.get("ML_PI") != "0" and pr["status"] != 3 and c["E"] >= 64:
                    assert ms["deferred_frames"] > 0, (name, S, knobs, ms)     # three to five schedules of >= 64 unknowns in 1024 words
            # codeword frames only: nothing flagged, ML_PI = 2 (no consistency test) allowed, ML_PI_IMAX on either side of I
            good = [f for f, k in enumerate(kinds) if k in ("codeword", "extra_parity", "all_clear")]
            xg, eg = np.ascontiguousarray(x[good]), np.ascontiguousarray(era[good])
            refg = tuple(np.ascontiguousarray(a[good]) for a in ref)
            n1 = int((want_st[good] == 1).sum())
            _configure(ctx, {})
            _same(ctx.decode(h, xg, eg), refg, (name, S, "codewords"))
            ms = ctx.ml_stats()
            assert ms["flagged_frames"] == 0 and ms["fast_path_frames"] == (n1 if fast_path else 0), (name, S, ms)
            _configure(ctx, {"ML_PI": "2"})
            _same(ctx.decode(h, xg, eg), refg, (name, S, "ML_PI=2"))
            I = mp.pi_inactivations(c)      # recorded from the fast path's model, asserted there by the CPU test
            if I is not None and pr["status"] == 1:
                for imax, fast in ((I, n1 if fast_path else 0), (I - 1, 0)):
                    _configure(ctx, {"ML_PI_IMAX": str(imax)})
                    _same(ctx.decode(h, xg, eg), refg, (name, S, "ML_PI_IMAX", imax))
                    assert ctx.ml_stats()["fast_path_frames"] == fast, (name, S, imax, ctx.ml_stats())
            if c["kind"] == "band" and c["w"] == 16 and c["E"] >= 40:   # a block no peeling gets through, 15 inactivations: not a fast-path frame at 8
                _configure(ctx, {"ML_PI_IMAX": "8"})
                _same(ctx.decode(h, xg, eg), refg, (name, S, "ML_PI_IMAX=8"))
                assert ctx.ml_stats()["fast_path_frames"] == 0, (name, S, ctx.ml_stats())
    finally:
        _configure(ctx, {})


def test_lds_and_global_scratch_arithmetic():
    """Where the matrix lives under ML_PACK = 4 (every case above runs that knob set): a workgroup then owns less than
    160 KB / 4 = 40 KB of LDS, part of it tables, and the matrix goes to LDS when nzr * W fits what is left, else to the global
    scratch.  (600,300), E = 300: 300 rows x 16 * 19 = 91 200 bytes (S = 1: 16 * 21, 100 800) -- more than the whole share:
    global scratch for certain.  E = 16, 16 rows: 16 x 16 = 256 bytes (S = 1: 16 x 48 = 768) -- of the 40 KB the tables of a
    300-check code take about 18 KB (the row lists 12 m, six 2 m or 3 m arrays, 9.5 KB of field tables, 4 m of levels): LDS."""
    big, small = mp.CASES["n600_circulant2_E300_top"], mp.CASES["n600_circulant2_E16_third"]
    for S in (1, 16):
        assert matrix_bytes(big["T"], big["E"], S) > 40 * 1024
        assert matrix_bytes(small["T"], small["E"], S) <= 4 * 1024
    assert matrix_bytes(300, 300, 16) == 91200 and matrix_bytes(300, 300, 1) == 100800 and matrix_bytes(16, 16, 1) == 768
    assert matrix_bytes(33, 33, 16) == 33 * 48 and matrix_bytes(32, 32, 1) == 32 * 48 and matrix_bytes(49, 49, 16) == 49 * 80


def _union_frames(oc, code, unions, S, rng, corrupt_every=3):
    """One frame per union of blocks (a codeword with those source columns erased; every `corrupt_every`-th one with a symbol of a
    touched check corrupted, the next one with a symbol only untouched checks see)."""
    sym, era, bad, props = [], [], [], {}
    for i, which in enumerate(unions):
        e = mp.erasures(code, which)
        pr = props.setdefault(tuple(which), mp.properties(code, e) if which else None)
        s = mp.erase(oc.encode(rng.integers(0, 256, size=(code.k, S), dtype=np.uint8)).reshape(code.n, S), e, int(rng.integers(256)))
        kind = "codeword"
        if which and i % corrupt_every == 1:
            tall = [r for b in which if code.plant[b]["kind"] in ("tall", "generic_tall") for r in code.plant[b]["rows"]]
            mp.corrupt_touched(rng, code, e, s, pr, rows=tall or None)      # (inside a surplus check where the union has some)
            kind = "touched"
        elif which and i % corrupt_every == 2:
            lo, hi = (pr["break_col"], pr["E"]) if pr["breaks"] else (None, None)
            if mp.corrupt_untouched(rng, code, e, s, pr, lo, hi) is not None:
                kind = "untouched"
        sym.append(s); era.append(e); bad.append(kind)
    return np.stack(sym), np.stack(era), bad


def _batch_against_the_oracle(ctx, oc, code, h, sym, era, kinds, S, what, knob_sets, need_deferred=True):
    exp = _oracle_frames(oc, sym, era, S)
    want_st = np.array([e[4] for e in exp])
    x = _shape(sym, S)
    _configure(ctx, {})
    ref = ctx.decode(h, x, era)
    ms = ctx.ml_stats()
    _equals_the_oracle(ref, exp, sym, era, S, what + ("default",))
    n_res = int(sum(1 for e in exp if 0 < e[3] <= code.m))
    assert ms["residual_frames"] == n_res, (what, ms, n_res)
    if S > 1:
        n_bad = sum(1 for f, k in enumerate(kinds) if k == "touched" and want_st[f] == 1 and _inconsistent(code, sym[f], era[f]))
        assert 0.8 * n_bad <= ms["flagged_frames"] <= n_bad, (what, ms, n_bad)
        assert 0 < ms["fast_path_frames"] <= int((want_st == 1).sum()), (what, ms)
        assert ms["residual_frames"] - ms["fast_path_frames"] >= int((want_st == 2).sum()) > 0, (what, ms)    # the exact path
    for knobs in knob_sets:
        _configure(ctx, knobs)
        _same(ctx.decode(h, x, era), ref, what + (tuple(knobs.items()),))
        ms2 = ctx.ml_stats()
        assert ms2["residual_frames"] == n_res, (what, knobs, ms2)
        if S > 1 and need_deferred and "ML_ARENA_WORDS" in knobs:
            assert ms2["deferred_frames"] > 0, (what, knobs, ms2)
    _configure(ctx, {})
    return ref, want_st, ms


def test_mixed_batch_every_family_every_size_class_in_both_orders(ctx, oracle):
    """One batch of one code holds every family: unions of the mixed code's blocks, 2 .. 300 unknowns -- all 16 size classes of the
    ML stage's work list --, all-clear frames and frames with more unknowns than checks, shuffled; F is no multiple of 64.  The
    same frames in reversed order give the same per-frame results."""
    code = mp.mixed_code()
    assert _max_col_degree(code) <= mp.DEVICE_COL_DEG
    oc = oracle.OracleCode(code)
    h = ctx.register_code(code)
    unions = mp.mixed_unions(code)
    sizes = [sum(code.plant[b]["E"] for b in w) for w in unions]
    assert {min(15, 16 * e // code.m) for e in sizes} == set(range(16)) and min(sizes) == 2 and max(sizes) == 300
    try:
        for S in (64, 1):
            rng = np.random.default_rng(4200 + S)
            sym, era, kinds = _union_frames(oc, code, unions + [[], [], []], S, rng)
            # more unknowns than checks: every source symbol + parity symbols, which no check can solve (each has two unknowns more)
            for extra in (1, 2, 7):
                e = mp.erasures(code)
                e[code.k + rng.choice(code.m, size=extra, replace=False)] = 1
                s = mp.erase(oc.encode(rng.integers(0, 256, size=(code.k, S), dtype=np.uint8)).reshape(code.n, S), e)
                sym, era, kinds = np.concatenate([sym, s[None]]), np.concatenate([era, e[None]]), kinds + ["too_many"]
            order = rng.permutation(sym.shape[0])
            sym, era, kinds = sym[order], era[order], [kinds[i] for i in order]
            F = sym.shape[0]
            assert F % 64 != 0 and F > 64, F
            knob_sets = [{"ML_PI": "0"}, {"ML_PACK": "4"}, {"ML_PACK": "1", "ML_THREADS": "1024"}, {"ML_ARENA_WORDS": "1024"},
                         {"ML_OVERLAP": "0"}, {"ML_SOLVE": "0"}, {"ML_SOLVE_B": "16"}] if S > 1 else KNOB_SETS_S1
            ref, want_st, ms = _batch_against_the_oracle(ctx, oc, code, h, sym, era, kinds, S, ("mixed", S), knob_sets)
            assert set(want_st.tolist()) == {0, 1, 2, 3}, np.bincount(want_st)
            if S > 1:
                assert ms["flagged_frames"] > 0, ms
            # LDS and global scratch in one launch (ML_PACK = 4 above): see test_lds_and_global_scratch_arithmetic
            assert matrix_bytes(300, 300, S) > 40 * 1024 and matrix_bytes(2, 2, S) <= 4 * 1024
            rev = ctx.decode(h, _shape(sym[::-1], S), np.ascontiguousarray(era[::-1]))
            _same(tuple(a[::-1] for a in rev), ref, ("mixed", S, "reversed"))
            # the library as shipped (ML_PI_ADAPTIVE left alone, a context of its own): after a batch without a frame for the ML stage
            # the next one skips the fast path; bytes and status words are the same either way (no counts asserted here)
            with api.Context(0) as fresh:
                h2 = fresh.register_code(code)
                quiet = np.zeros((3, code.n), dtype=np.uint8)
                fresh.decode(h2, _shape(sym[:3], S), quiet)
                fresh.synchronize()
                for _ in range(2):
                    _same(fresh.decode(h2, _shape(sym, S), era), ref, ("mixed", S, "shipped defaults"))
    finally:
        _configure(ctx, {})


def test_long_batches_factor_many_systems_on_one_workgroup(ctx, oracle):
    """S = 1, more than 3 x 1024 frames, ML_PACK = 4: the frames alternate 272 unknowns in 284 checks (a generic block with surplus checks + a
    band, 15 inactivations deep + a 2 x 2 block) / 14 unknowns / a rank-deficient 16-unknown block whose second column is a multiple
    of the first / all clear, so every workgroup factors several systems one after the other on the same LDS -- where stale perm,
    colmap, counters or keys would show.  Frames corrupted inside a surplus check are inconsistent: their bytes depend on the
    pivot order at S = 1, and the fast path must flag them at S = 16.  Then the same at S = 16 with more than two frames per CU."""
    import torch
    code = mp.long_code()
    assert _max_col_degree(code) <= mp.DEVICE_COL_DEG
    oc = oracle.OracleCode(code)
    h = ctx.register_code(code)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pattern = [[0, 1, 2], [0, 2], [3], None]
    try:
        for S, F in ((1, 3 * 1024 + 4 + 1), (16, 2 * cus + 4 + 1)):
            rng = np.random.default_rng(4300 + S)
            sym, era, kinds = _union_frames(oc, code, [pattern[i % 4] or [] for i in range(F)], S, rng, corrupt_every=5)
            assert F % 64 != 0 and (S > 1 or F >= 3 * 1024) and (S == 1 or F >= 2 * cus)
            knob_sets = [{"ML_PACK": "4"}, {"ML_PACK": "4", "ML_THREADS": "1024"}, {"ML_PACK": "1"}] if S == 1 else \
                [{"ML_PACK": "4"}, {"ML_PI": "0", "ML_PACK": "4"}, {"ML_ARENA_WORDS": "1024"}, {"ML_OVERLAP": "1"}, {"ML_PI": "0", "ML_SOLVE": "0"}]
            ref, want_st, ms = _batch_against_the_oracle(ctx, oc, code, h, sym, era, kinds, S, ("long", S), knob_sets)
            assert np.bincount(want_st, minlength=3)[:3].min() >= F // 4 - 1, np.bincount(want_st)
            assert "untouched" in [k for k, st in zip(kinds, want_st) if st == 2]      # zero-row right-hand sides that are not zero
            if S > 1:
                assert ms["flagged_frames"] > 0, ms
            # the 272-unknown system is 284 rows x 16 * 17 (S = 1: 16 * 19) = 77 248 (86 336) bytes: global scratch at ML_PACK = 4;
            # the 14- and 16-unknown ones (26 x 16, 16 x 16; S = 1: x 48) are in LDS
            assert matrix_bytes(284, 272, S) == 284 * (304 if S == 1 else 272) > 40 * 1024 and matrix_bytes(26, 14, S) <= 26 * 48
    finally:
        _configure(ctx, {})
