"""tools/step_patterns.py against the oracle alone (no GPU): the patterns tests/test_gpu_plan_edges.py places on the packet kernels'
thresholds have the property they were built for, and the numpy reference of one in-order sweep gives the oracle's bytes.

  * parity-only patterns: exactly t parity symbols erased -> one sweep, nothing left, status 0, for t at the ends, around a
    wavefront (63, 64, 65) and at random, in every placement, on the built-in triangle codes;
  * single_sweep_reference == oracle.decode_packets byte for byte on symbols that are NO codeword (so "equals the codeword" cannot
    stand in for it), on the (2040,1530) code and on a small hand-made triangle code;
  * exact-E sets: at least 95 % of the frames E = 0 .. 0.18 n peel completely.  This is a condition on the INPUTS of the GPU test
    (its frames are meant to have E steps and no ML stage), not a measurement: if a seed falls under it, change the seed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import step_patterns as sp  # noqa: E402

from ldpc_erasure_codes_amd import codes  # noqa: E402

CODE_INDS = [1, 2] + ([3] if codes.have_builtin(3) else [])
F2_SEED = 20                      # the seed tests/test_gpu_plan_edges.py draws its exact-E frames with


def _ts(m, seed):
    rng = np.random.default_rng(seed)
    return [0, 1, 2, 63, 64, 65, m - 1, m] + sorted(int(t) for t in rng.choice(np.arange(3, m - 1), size=20, replace=False))


@pytest.mark.parametrize("ci", CODE_INDS)
def test_parity_patterns_take_one_sweep_and_leave_nothing(oracle, ci):
    code = codes.load_builtin(ci)
    assert sp.is_triangle(code)
    oc = oracle.OracleCode(code)
    m = code.n - code.k
    ts = _ts(m, 100 + ci)
    rows = [(t, w) for t in ts for w in sp.WHERE]
    era = np.stack([sp.parity_subset(code, t, 11, w) for t, w in rows])
    assert np.array_equal(era.sum(1), [t for t, _ in rows]) and not era[:, :code.k].any()
    first = era[[w == "first" for _, w in rows]]
    last = era[[w == "last" for _, w in rows]]
    for t, f, l in zip(ts, first, last):
        assert f[code.k:code.k + t].all() and l[code.n - t:].all()
    src = oracle.synth_source(3 + ci, 0, 1, code.k, 1)[0, :, 0]
    cw = oc.encode(src)
    sym = np.repeat(cw[None], len(rows), axis=0)
    sym[era.astype(bool)] = 0x5A
    out, sw, res, st = oc.decode_batch_s1(sym, era)
    bad = [(rows[i], int(sw[i]), int(res[i]), int(st[i])) for i in range(len(rows)) if sw[i] != 1 or res[i] != 0 or st[i] != 0]
    assert not bad, bad
    assert np.array_equal(out, np.repeat(cw[None], len(rows), axis=0))


def _reference_equals_oracle(oracle, code, F, S, seed):
    oc = oracle.OracleCode(code)
    m = code.n - code.k
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 256, size=(F, code.n, S), dtype=np.uint8)     # no codeword
    ts = [m, m - 1, m // 2, 1] + [int(t) for t in rng.integers(2, m - 1, size=max(0, F - 4))]
    era = np.stack([sp.parity_subset(code, t, seed + f, sp.WHERE[f % 3]) for f, t in enumerate(ts[:F])])
    sym[era.astype(bool)] = 0x5A
    ref = sp.single_sweep_reference(code, sym, era)
    assert np.array_equal(ref[~era.astype(bool)], sym[~era.astype(bool)])          # received symbols pass through
    for f in range(F):
        out, oe, it, info, rc = oc.decode_packets(sym[f], era[f])
        assert it == 1 and info[0] == 0 and not oe.any(), (f, ts[f])
        assert np.array_equal(ref[f], out), (f, ts[f])
    # what the erased symbols held on the way in is never read
    sym2 = sym.copy()
    sym2[era.astype(bool)] = 0xC3
    assert np.array_equal(sp.single_sweep_reference(code, sym2, era), ref)


def test_reference_equals_oracle_on_the_builtin_code(oracle, code_a):
    _reference_equals_oracle(oracle, code_a, F=8, S=16, seed=41)


def test_reference_equals_oracle_on_a_hand_made_triangle(oracle):
    code = sp.triangle_code(130, 66, 20)
    assert sp.is_triangle(code) and (np.diff(code.row_ptr.astype(np.int64))[2:] == 20).all()
    _reference_equals_oracle(oracle, code, F=4, S=16, seed=43)


def test_reference_refuses_what_it_does_not_cover(code_a):
    sym = np.zeros((1, code_a.n, 4), dtype=np.uint8)
    era = np.zeros((1, code_a.n), dtype=np.uint8)
    era[0, 5] = 1                                                                   # a source symbol
    with pytest.raises(ValueError):
        sp.single_sweep_reference(code_a, sym, era)
    with pytest.raises(ValueError):
        sp.parity_subset(code_a, code_a.n - code_a.k + 1, 0)
    with pytest.raises(ValueError):
        sp.parity_subset(code_a, 3, 0, "middle")


def test_exact_sets_peel_completely_up_to_018n(oracle, code_a):
    oc = oracle.OracleCode(code_a)
    n = code_a.n
    Es = list(range(0, int(np.floor(0.18 * n)) + 1))
    era = np.stack([sp.exact_subset(code_a, E, F2_SEED) for E in Es])
    assert np.array_equal(era.sum(1), Es)
    _, sw, res, st = oc.decode_batch_s1(np.zeros((len(Es), n), dtype=np.uint8), era, itenum=10, do_ml=0)
    peeled = (res == 0) & (st == 0)
    assert peeled.mean() >= 0.95, (float(peeled.mean()), [Es[i] for i in np.flatnonzero(~peeled)])
    assert sw[1:].min() >= 1 and sw.max() > 1                                        # these frames need more than one sweep
