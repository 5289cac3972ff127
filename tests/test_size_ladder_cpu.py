"""The size ladder (tools/size_ladder.py) pinned on the CPU oracle alone: every code is what register_code documents as valid input
and is in triangle form, every batch holds the frame kinds it claims, with the step counts it claims, and the flags really carry all
four non-zero values.  tests/test_gpu_size_ladder.py then takes the same codes and batches through the kernels.

Measured: building all 17 codes and batches and the oracle's side of this file (S = 16; max_sweeps 10 with the ML stage on and off,
max_sweeps 1) take 2.7 s, the whole file from the set-up of its first test to its last test 3.0 s.  BOUND_S below is about ten times that; the last
test asserts it on the whole file: a slow machine passes, a ladder that has grown to minutes does not."""
import time

import numpy as np
import pytest

import size_ladder_cases as cases
from size_ladder_cases import sl

BOUND_S = 40.0
S = 16
_SPENT = {}
_CLOCK = {}


@pytest.fixture(scope="module", autouse=True)
def file_clock():
    """the file's clock: from the set-up of its first test (modules are imported long before, at collection) to its last test"""
    _CLOCK["t0"] = time.perf_counter()


@pytest.fixture(scope="module", params=[r.name for r in sl.RUNGS])
def rung(request, oracle):
    t0 = time.perf_counter()
    c = cases.rung_case(request.param)
    cases.symbols(request.param, S)
    for ms, ml in ((10, 1), (10, 0), (1, 1)):
        cases.want(request.param, S, ms, ml)
    _SPENT.setdefault(request.param, time.perf_counter() - t0)
    return c


def test_code_is_valid_input_in_triangle_form(rung):
    code, facts, r = rung["code"], rung["facts"], rung["rung"]
    assert (code.n, code.m) == (r.n, r.m) and 1 < code.n <= 65534 and 1 <= code.k < code.n
    assert code.row_ptr[0] == 0 and code.row_ptr[-1] == code.cols.size == code.coefs.size
    assert facts["ascending"] and int(code.cols.max()) < code.n and int(code.coefs.min()) >= 1
    assert facts["triangle"]
    assert facts["maxdeg"] == r.deg <= 24 and facts["mindeg"] >= r.deg - 1      # d14: 13 or 14 entries per check; the banded d16 rung: 16
    assert facts["maxcoldeg"] <= 16                                             # light columns: the packet kernel, not the gather kernel, where it fits
    # the planted columns are where the docstring says, and in no other check
    p = rung["planted"]
    rp, cols = code.row_ptr.astype(np.int64), code.cols.astype(np.int64)
    holders = lambda j: sorted(int(np.searchsorted(rp, e, side="right") - 1) for e in np.flatnonzero(cols == j))  # noqa: E731
    assert all(holders(j) == p["g_checks"] for j in p["G"])
    c3, c2, c1 = p["h_checks"]
    assert c3 < c2 < c1 and [holders(j) for j in p["H"]] == [[c2, c1], [c3, c2], [c3]]
    assert holders(p["Z"]) == []


def test_batch_holds_the_frame_kinds_it_claims(rung):
    b, code, name = rung["batch"], rung["code"], rung["rung"].name
    m, k = code.m, code.k
    F = len(b.kinds)
    assert F <= 9 and b.flags.shape == (F, code.n)
    w = cases.want(name, S, 10, 1)
    sym, cw = cases.symbols(name, S)["sym"], cases.symbols(name, S)["cw"]
    changed = {f for f, _, _ in b.corrupt}
    f0 = b.kinds.index("none")
    assert not b.flags[f0].any() and f0 not in changed                        # an unerased codeword: it comes back as it went in
    assert w.status[f0] == 0 and np.array_equal(w.out[f0], sym[f0]) and np.array_equal(sym[f0], cw[f0])
    # parity only, exactly t steps in one sweep: on both sides of 2 * 256 and 2 * 512 (as far as m goes), and t = m
    ts = [t for t in b.steps if t is not None]
    assert set(ts) == {min(t, m) for t in (511, 513, 1023, 1025)} | {m}
    for f, t in enumerate(b.steps):
        if t is None:
            continue
        assert not b.flags[f, :k].any() and int((b.flags[f] != 0).sum()) == t
        assert (w.sweeps[f], w.residual[f], w.status[f]) == (1, 0, 0)
        if f not in changed:
            assert np.array_equal(w.out[f], cw[f])
        else:                                                                 # no codeword: the sweeps' bytes are not the encoder's
            assert not np.array_equal(w.out[f], cw[f]) and np.array_equal(w.out[f][b.flags[f] == 0], sym[f][b.flags[f] == 0])
    assert any(f in changed for f, t in enumerate(b.steps) if t is not None), "no parity-only frame that is no codeword"
    # message passing completes in three sweeps; with one sweep two symbols are left and the ML stage solves them
    f3 = b.kinds.index("sweeps3")
    assert (w.sweeps[f3], w.residual[f3], w.status[f3]) == (3, 0, 0) and np.array_equal(w.out[f3], cw[f3])
    w1 = cases.want(name, S, 1, 1)
    assert (w1.sweeps[f3], w1.residual[f3], w1.status[f3]) == (1, 2, 1) and np.array_equal(w1.out[f3], cw[f3])
    # the ML stage solves the planted 4 x 4 system
    fm = b.kinds.index("ml")
    assert (w.residual[fm], w.status[fm]) == (4, 1) and np.array_equal(w.out[fm], cw[fm])
    # rank deficient (status 2) or more unknowns than checks (status 3)
    if "deficient" in b.kinds:
        fd = b.kinds.index("deficient")
        assert (w.residual[fd], w.status[fd]) == (1, 2) and w.erased_out[fd].sum() == 1 and w.residual_src[fd] == 1
    else:
        fa = b.kinds.index("all")
        assert w.residual[fa] > m and w.status[fa] == 3 and np.array_equal(w.erased_out[fa], b.flags01[fa])
    assert set(w.status.tolist()) >= {0, 1} and set(w.status.tolist()) & {2, 3}
    # ML off: whatever the sweeps leave is status 3
    w0 = cases.want(name, S, 10, 0)
    assert set(w0.status.tolist()) == {0, 3} and np.array_equal(w0.sweeps, w.sweeps) and np.array_equal(w0.residual, w.residual)


def test_flags_carry_all_four_nonzero_values(rung):
    b = rung["batch"]
    assert set(np.unique(b.flags).tolist()) == {0} | set(sl.FLAG_VALUES)
    assert set(np.unique(b.flags01).tolist()) == {0, 1} and np.array_equal(b.flags01 != 0, b.flags != 0)
    for f in range(len(b.kinds)):
        if int((b.flags[f] != 0).sum()) >= 64:
            assert set(np.unique(b.flags[f]).tolist()) == {0} | set(sl.FLAG_VALUES), b.kinds[f]


def test_ladder_has_both_open_frame_kinds_and_every_named_switch():
    kinds = {k for r in sl.RUNGS for k in cases.rung_case(r.name)["batch"].kinds}
    assert {"deficient", "all"} <= kinds
    assert len({r.name for r in sl.RUNGS}) == len(sl.RUNGS) and all(r.switch for r in sl.RUNGS)
    assert [r.n * 1 for r in sl.RUNGS] == sorted(r.n for r in sl.RUNGS), "smallest first: the GPU test runs the rungs in this order"


def test_host_arithmetic_refuses_nothing_inside_the_claimed_envelope():
    """tools/size_ladder.host_plan, the mirror of the host half of csrc/kernels.hip the refused list of the GPU test is checked
    against: n <= 8192 and m <= 4096 with row degree up to 16 is served by decode and encode at S = 1 and on packets, ML on or off."""
    for r in sl.RUNGS:
        if r.n > 8192 or r.m > 4096:
            continue
        f = cases.rung_case(r.name)["facts"]
        for entry in ("encode", "decode", "decode_frames", "inplace"):
            for s in (1, 16, 256):
                if entry == "inplace" and s == 1:
                    continue
                for ml in (0, 1):
                    p = sl.host_plan(r.n, r.m, f["maxdeg"], f["maxcoldeg"], entry, s, 10, ml)
                    assert p["refused"] is None, (r.name, entry, s, ml, p)
    # ... and the d14 rung is the one whose serial peel plan does not fit while the relaxation's does
    p = sl.host_plan(8192, 4096, 14, 12, "decode", 16, 10, 1)
    assert p["peel"] == "relax" and p["tables_in_global"] and sl._peel_lds(8192, 4096, 4096, 14, False, False) == 172048 > sl.LDS_MAX


def test_the_ladder_stays_quick():
    assert len(_SPENT) == len(sl.RUNGS)
    whole = time.perf_counter() - _CLOCK["t0"]
    print("size ladder: codes, batches and oracle %.1f s, the whole file %.1f s" % (sum(_SPENT.values()), whole))
    assert whole < BOUND_S
