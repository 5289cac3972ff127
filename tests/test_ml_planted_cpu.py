"""Planted residual systems (tools/ml_plant.py) on the CPU: the generator's inputs do what they were designed to do, and the three
restatements of the reference's elimination (Matlab/My_LDPC_HybridML_NonBinary_Erasure_Decoder.m:61-128) agree on them.
  * every case the GPU test (tests/test_gpu_ml_planted.py) runs has its DESIGNED property, computed by ml_plant.properties from
    the reference's rule: the block is what the sweeps leave; `anti` at the bottom displaces the pivot of every column and every
    swap moves an all-zero row; dupcol(c) breaks at column c + 1, circulant2_singular at the last column, wide somewhere;
    dense / band / tall are full rank; the cases at m = 4096 take their pivots from rows >= 4000.  An input that stopped hitting
    its edge fails here instead of silently testing the generic case;
  * oracle/oracle.c = properties in status, residual count and iterations on every case and kind of frame;
  * oracle/oracle.c = tests/matlab_literal.py byte for byte and in `iterations` on every case with E <= 64 -- codewords, a symbol
    corrupted inside a touched check, one corrupted inside untouched checks only, the four cases at (8192,4096) included;
  * tools/pi_model.py returns the oracle's bytes on the full-rank codeword frames; its inactivation count per family is recorded
    in ml_plant.pi_inactivations -- the GPU test sets ML_PI_IMAX on either side of it;
  * the right-hand side of an all-zero row IS observable: on the rank-deficient cases at the bottom, corrupting a symbol that
    only untouched checks see changes the bytes the oracle writes back."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ml_plant as mp  # noqa: E402
import pi_model  # noqa: E402

import matlab_literal as lit  # noqa: E402

CASES = list(mp.CASES)



def _recv(sym, era):
    recv = sym.astype(np.int16)
    recv[era != 0] = -1
    return recv


def _status(info, rc):
    return 0 if info[0] == 0 else (3 if (rc == -2 or not info[1]) else (2 if info[2] else 1))


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name):
        if name not in cache:
            code = mp.case_code(name)
            cache[name] = (code, mp.properties(code, mp.erasures(code)))
        return cache[name]
    return get


@pytest.mark.parametrize("name", CASES)
def test_the_case_has_its_designed_property(built, name):
    c = mp.CASES[name]
    code, pr = built(name)
    m, E, T, kind, where = code.m, c["E"], c["T"], c["kind"], c["where"]
    rows = mp.placement(m, T, where)
    # the sweeps leave exactly the block, embedded at the chosen rows
    assert pr["E0"] == pr["E"] == E and pr["T"] == T and pr["iterations"] == 10, pr
    assert np.array_equal(pr["residual_cols"], np.arange(E)) and np.array_equal(pr["touched"], rows), pr
    assert int(np.diff(code.row_ptr.astype(np.int64)).max()) <= mp.DEVICE_ROW_DEG
    if E > m:
        assert pr["status"] == 3 and E == m + 1, pr
        return
    done = pr["break_col"] if pr["breaks"] else E             # columns that found a pivot
    if kind in mp.FULL_RANK:
        assert pr["status"] == 1 and not pr["breaks"], pr
    elif kind == "dupcol":
        assert pr["status"] == 2 and pr["break_col"] == c["c"] + 1, pr
    elif kind in ("circulant2_singular", "generic_singular"):
        assert pr["status"] == 2 and pr["break_col"] == E - 1, pr
    else:
        assert kind == "wide" and pr["status"] == 2 and pr["break_col"] <= T, pr
    if where == "bottom" and m - T >= E:
        # every pivot search skips the zero rows above the block, and every swap sends an all-zero row down
        assert pr["displaced"] == done and pr["zero_row_swaps"] == done, pr
        assert pr["max_pivot_row"] >= m - T, pr
    if kind == "anti":
        if where == "bottom" and m - T >= E:
            assert pr["displaced"] == E and pr["zero_row_swaps"] >= E and pr["max_pivot_row"] == m - 1, pr
        else:
            assert pr["displaced"] >= E // 2 - 1 and pr["max_pivot_row"] >= rows[E - 2], pr     # column 0 pivots at the far end
    if kind.startswith("generic"):
        # generic pivoting: non-zero rows are swapped down and compete again -- a search that took the smallest STORED row would differ
        assert pr["not_min_stored"] > 0 and pr["displaced"] > pr["zero_row_swaps"], pr
    if kind in ("tall", "generic_tall"):
        assert T > E and pr["touched"].size - E >= E, pr       # surplus non-zero rows are left below the pivots
    if kind == "circulant2" and where == "top":
        assert pr["displaced"] == 0, pr                        # the on-diagonal baseline
    if m == 4096 and where == "clusters":
        assert rows[-1] >= 4000 > rows[0] and pr["max_pivot_row"] >= 4000 and pr["not_min_stored"] > 0, pr
    elif m == 4096:
        assert rows[0] >= 4000 and pr["max_pivot_row"] >= 4000 and pr["displaced"] == done, pr   # 12-bit fields near 4095
    if name.startswith("n100_"):
        assert E == m and pr["status"] == 1, pr                # as many unknowns as checks


def test_the_edges_are_all_there():
    seen = {(c["kind"], c["where"]) for c in mp.CASES.values()}
    for kind in ("circulant2", "anti"):
        for where in mp.WHERE:
            assert (kind, where) in seen, (kind, where)
        assert {c["E"] for c in mp.CASES.values() if c["kind"] == kind and c["n"] == 600} == set(mp.E_EDGES)
    assert {c["c"] for c in mp.CASES.values() if c["kind"] == "dupcol" and c["E"] == 64 and c["n"] == 600} == {0, 32, 62}
    assert {c["kind"] for c in mp.CASES.values() if c["n"] == 8192} >= {"anti", "dupcol", "tall", "circulant2_singular"}
    assert {c["kind"] for c in mp.CASES.values()} == {"circulant2", "circulant2_singular", "anti", "dense", "band", "dupcol", "wide", "tall",
                                                          "generic", "generic_singular", "generic_tall"}


def _frames(oc, code, pr, seed):
    """The frames of ml_plant.case_frames at S = 1: [(kind of frame, symbols [n], erasure flags [n], the frame's codeword [n])]."""
    sym, era, kinds, cw = mp.case_frames(oc, code, pr, 1, seed, codewords=True)
    return [(k, sym[f, :, 0], era[f], cw[f, :, 0]) for f, k in enumerate(kinds)]


@pytest.mark.parametrize("name", CASES)
def test_oracle_properties_literal_model_and_fast_path_model_agree(oracle, built, name):
    c = mp.CASES[name]
    code, pr0 = built(name)
    oc = oracle.OracleCode(code)
    frames = _frames(oc, code, pr0, 500 + CASES.index(name))
    H = code.dense() if c["E"] <= 64 else None
    prepared = lit.prepare(H) if H is not None and code.n > 2048 else None     # (8192,4096): the code's side once for the three frames
    kinds = [k for k, _, _, _ in frames]
    assert "codeword" in kinds and "touched" in kinds and "all_clear" in kinds
    assert "untouched" in kinds or c["T"] >= code.m - 2, kinds            # (no untouched check to speak of: nothing to corrupt)
    assert "extra_parity" in kinds or c["T"] == code.m, kinds
    for kind, sym, era, cw in frames:
        what = (name, kind)
        pr = mp.properties(code, era)
        msg, it, info, rc = oc.decode(_recv(sym, era))
        assert (int(info[0]), _status(info, rc), it) == (pr["E"], pr["status"], pr["iterations"]), (what, info, rc, it, pr)
        if kind == "extra_parity":
            assert pr["E0"] > pr["E"] == c["E"] and np.array_equal(pr["touched"], pr0["touched"]), what   # the residual is still the block
        if kind == "all_clear":
            assert pr["status"] == 0 and it == 1 and np.array_equal(msg, cw), what
        if pr["status"] == 1 and kind in ("codeword", "untouched", "extra_parity"):
            assert np.array_equal(msg[era != 0], cw[era != 0]), what   # a consistent full-rank system has ONE solution
        if H is not None and kind in ("codeword", "touched", "untouched"):
            if pr["status"] == 3:      # E = m + 1: the write-back rhs(1:E) runs off the m right-hand sides, Matlab stops with an error (:127)
                with pytest.raises(IndexError):
                    lit.hybridml_nonbinary_decode(_recv(sym, era), H)
                continue
            m2, it2, dj = lit.hybridml_nonbinary_decode(_recv(sym, era), H, prepared=prepared)
            assert it2 == it and np.array_equal(m2, msg) and dj == int(info[2]), (what, dj, info)
        if kind == "codeword" and pr["status"] == 1:
            levels, nslots, inf = pi_model.build_schedule(code, era.astype(bool), verify=True)
            got, consistent = pi_model.run_schedule(levels, nslots, sym.reshape(-1, 1).copy())
            assert consistent and np.array_equal(got[:, 0], msg.astype(np.uint8)), (what, inf)
            assert inf["P"] + inf["I"] == c["E"], (what, inf)
            want = mp.pi_inactivations(c)
            assert want is None or inf["I"] == want, (what, inf["I"], want)
        if kind == "codeword" and pr["status"] == 2:
            with pytest.raises(pi_model.NeedExactPath):
                pi_model.build_schedule(code, era.astype(bool), verify=True)


def test_dense_block_of_64_on_the_oracle_alone(oracle):
    """All 64 x 64 entries (rows of 68 entries: more than the library registers, so this one stays on the CPU), at the bottom:
    ML ran, full rank; 50 x 64: rank deficient; both equal the literal model; the fast path's model inactivates E - 1."""
    rng = np.random.default_rng(64)
    for T, want in ((64, [64, 1, 0]), (50, [64, 1, 1])):
        code = mp.plant(rng, 600, 300, 64, mp.placement(300, T, "bottom"), "dense", device=False)
        oc = oracle.OracleCode(code)
        era = mp.erasures(code)
        cw = oc.encode(rng.integers(0, 256, size=code.k, dtype=np.uint8))
        sym = mp.erase(cw, era)
        msg, it, info, rc = oc.decode(_recv(sym, era))
        assert info.tolist() == want and it == 10
        m2, it2, dj = lit.hybridml_nonbinary_decode(_recv(sym, era), code.dense())
        assert it2 == it and np.array_equal(m2, msg) and dj == want[2]
        if T == 64:
            assert np.array_equal(msg.astype(np.uint8), cw)
            assert pi_model.build_schedule(code, era.astype(bool))[2]["I"] == 63


RANK_DEFICIENT_AT_THE_BOTTOM = [n_ for n_, c_ in mp.CASES.items()
                                if c_["where"] == "bottom" and c_["kind"] in ("dupcol", "wide", "circulant2_singular")
                                and c_["n"] - c_["k"] - c_["T"] >= c_["E"]]


@pytest.mark.parametrize("name", RANK_DEFICIENT_AT_THE_BOTTOM)
def test_the_right_hand_side_of_a_zero_row_is_observable(oracle, built, name):
    """Rank deficient, block at the bottom: the logical positions break_col..E-1 still hold all-zero rows when the elimination
    stops, and :127 writes their right-hand sides back.  A corrupted symbol that only such checks see changes those bytes."""
    code, pr = built(name)
    assert pr["status"] == 2
    oc = oracle.OracleCode(code)
    rng = np.random.default_rng(700 + CASES.index(name))
    era = mp.erasures(code)
    cw = oc.encode(rng.integers(0, 256, size=code.k, dtype=np.uint8))
    sym = mp.erase(cw, era)
    bad = sym.copy()
    j = mp.corrupt_untouched(rng, code, era, bad, pr, pr["break_col"], pr["E"])
    assert j is not None, "no symbol that only the written-back zero rows see"
    a = oc.decode(_recv(sym, era))[0]
    b = oc.decode(_recv(bad, era))[0]
    differ = np.flatnonzero(a != b)
    differ = differ[differ != j]
    assert differ.size >= 1 and (era[differ] == 1).all(), (name, differ)


def test_mixed_and_long_codes(oracle):
    """The codes of the GPU test's mixed and long batches: every block alone has its designed rank, unions of the mixed code's
    blocks reach all 16 size classes of the ML stage's work list (class = 16 * unknowns / m, the last one from 15/16 m on)."""
    code = mp.mixed_code()
    assert [p["kind"] for p in code.plant] == [b[0] for b in mp.MIXED_BLOCKS] and sum(p["E"] for p in code.plant) == code.k == 300
    oc = oracle.OracleCode(code)
    classes = set()
    for which in mp.mixed_unions(code):
        era = mp.erasures(code, which)
        pr = mp.properties(code, era)
        assert pr["E"] == pr["E0"] == sum(code.plant[b]["E"] for b in which), which      # the sweeps solve nothing of a union
        classes.add(min(15, 16 * pr["E"] // code.m))
        _, it, info, rc = oc.decode(_recv(np.zeros(code.n, dtype=np.uint8), era))
        assert (int(info[0]), _status(info, rc)) == (pr["E"], pr["status"]), which
    assert classes == set(range(16)), sorted(classes)
    lc = mp.long_code()
    prs = [mp.properties(lc, mp.erasures(lc, w)) for w in ([0, 1, 2], [0, 2], [3])]
    assert [p["status"] for p in prs] == [1, 1, 2] and prs[2]["break_col"] == 1
    assert prs[0]["not_min_stored"] > 0 and prs[1]["not_min_stored"] > 0 and prs[0]["T"] > prs[0]["E"] == 272
