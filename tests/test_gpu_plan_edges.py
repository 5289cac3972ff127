"""The packet kernels at EVERY step count across the edges of their launch plans ("Plan edges").

ldpc_scatter_kernel / ldpc_scatter_big_kernel, their packets-in forms and the schedules the peel kernels write for them switch
behaviour on a frame's number of solved steps (sched_hdr[2 f]) at hard thresholds:
  * nsteps > tier1_cap: tier 1 or tier 2 (written in the peel kernel, in the relaxation and in tier 1's early return: a frame the
    three disagree about is decoded by no tier);
  * nsteps (B + 4 cdw) <= nslots B: the level phase's column lists fit the LDS behind the accumulators, or stay in global memory;
  * nsteps (B + 4 cdw + 10) + 16 <= nslots B: the pull records fit too and the levels run in pairs;
  * the register-held set-up (2 steps, 2 list words, 4 symbols per thread) against the loops behind it: nsteps across nthr and
    2 nthr, nsteps cdw across 2 nthr, with 256, 512 and 1024 threads;
  * tier1_cap itself moves with SCATTER_B, SCATTER_TIERS and the packets-in plan.
A channel deals step counts at random.  tools/step_patterns.py CHOOSES them: erasing t parity symbols of a triangle-form code gives
exactly t steps in one sweep, so a batch with one frame per t = 0 .. m puts a frame on every threshold of every plan, whatever the
knobs make of it.  tests/test_step_patterns_cpu.py pins the patterns and the numpy reference on the oracle.

Families:  F1 parity-only, every t, even frames codewords and odd frames random bytes (expected: tools/step_patterns.py
single_sweep_reference; sweeps 1, residual 0, status 0);  F2 exactly E symbols of all n erased, E = 0 .. 0.18 n, codewords
(sweeps / residual / status from the oracle on the pattern; bytes = the codeword where the oracle's status is 0 or 1, elsewhere
byte lanes 0 and S - 1 = the oracle's S = 1 decode of the lane), also with the sweeps capped at 1 and 2 so that the ML stage writes
back behind both tiers;  F3 heavy, E = 0.19 n .. 0.23 n: residual frames behind step counts where lists and pull records stop fitting.

Every output buffer is filled with 0xA5 before every call: a frame no tier writes must not inherit an earlier run's correct bytes.
Comparisons run on the device; a mismatch names the frames and their step counts."""
import os
import sys

import numpy as np
import pytest

from ldpc_erasure_codes_amd import api, codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import step_patterns as sp  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = 0xA5
POISON32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
ERASED_FILL = 0x5A                      # what an erased symbol holds on the way in: never read
F1_SEED, F2_SEED, F3_SEED = 10, 20, 30  # (F2_SEED: tests/test_step_patterns_cpu.py checks that these frames peel)
# name -> (built-in code, S, threads per workgroup, two tiers, bytes of every row per workgroup)
BATCHES = {"A256": (1, 256, 1024, 1, 256), "A16": (1, 16, 256, 0, 16), "C128": (3, 128, 1024, 1, 128), "B64": (2, 64, 512, 0, 64)}
KNOBS = ["SCATTER_B", "SCATTER_TIERS", "SCATTER_PAIRS", "SCATTER_XL", "SCATTER_LISTS", "SCATTER_DYN", "SCATTER_NT", "SCATTER_T2B",
         "SCATTER_T2P", "SCATTER_R2", "PEEL_RELAX", "APPLY"]
VARIANTS = [("SCATTER_B", "128"), ("SCATTER_B", "64"), ("SCATTER_TIERS", "1"), ("SCATTER_PAIRS", "0"), ("SCATTER_XL", "0"),
            ("SCATTER_LISTS", "1"), ("SCATTER_DYN", "0"), ("SCATTER_DYN", "2"), ("SCATTER_DYN", "3"), ("SCATTER_DYN", "4"),
            ("SCATTER_NT", "0"), ("SCATTER_T2B", "128"), ("PEEL_RELAX", "0"), ("APPLY", "gather")]


@pytest.fixture(scope="module")
def ctx():
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("LDPC_AMD_")}
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()
    _CACHE.clear()
    os.environ.update(saved)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Family:
    """One family of one batch: inputs on the device, expectations on the device, the outputs of the default run once it ran."""

    def __init__(self, name, sym, era, cw, steps):
        self.name, self.sym, self.cw, self.steps = name, sym, cw, np.asarray(steps)
        self.era_host = era
        self.era = _dev(era)
        self.F = sym.shape[0]
        self.want = {}        # (max_sweeps, do_ml) -> dict(out=, good=, lanes=, sweeps=, residual=, status=)
        self.default = None   # the default plan's four outputs
        self.bufs = None

    def buffers(self):
        """The family's output buffers, recycled from call to call and filled with the poison before each."""
        if self.bufs is None:
            self.bufs = (torch.empty_like(self.sym),) + tuple(torch.empty((self.F,), dtype=torch.int32, device="cuda") for _ in range(3))
        self.bufs[0].fill_(POISON)
        for b in self.bufs[1:]:
            b.fill_(POISON32)
        return self.bufs


def differing(got, want):
    """Frames (first axis) in which two device tensors differ."""
    return (got != want).reshape(got.shape[0], -1).any(1).nonzero().flatten().tolist()


def assert_same(got, want, steps, tag):
    if got.shape == want.shape and torch.equal(got, want):
        return
    assert got.shape == want.shape, (tag, tuple(got.shape), tuple(want.shape))
    bad = differing(got, want)
    raise AssertionError(f"{tag}: {len(bad)} of {got.shape[0]} frames differ: "
                         + ", ".join(f"frame {f} (steps {int(steps[f])})" for f in bad[:24]))


def check_family(fam, outs, key, tag):
    """The four outputs of a decode of `fam` against the expectation `key` = (max_sweeps, do_ml)."""
    w = fam.want[key]
    steps = w.get("steps", fam.steps)      # (under a sweep cap a frame has fewer steps than under the default)
    out, sw, res, st = outs
    assert_same(sw, w["sweeps"], steps, f"{tag} {fam.name} sweeps")
    assert_same(res, w["residual"], steps, f"{tag} {fam.name} residual")
    assert_same(st, w["status"], steps, f"{tag} {fam.name} status")
    if w["good"] is None:
        assert_same(out, w["out"], steps, f"{tag} {fam.name} bytes")
    else:
        g = w["good"]
        assert_same(out[g], w["out"][g], steps[g.cpu().numpy()], f"{tag} {fam.name} bytes")
        for f, lane, ref in w["lanes"]:     # rank-deficient frames: byte lanes against the oracle's S = 1 decode of the lane
            assert torch.equal(out[f, :, lane], ref), f"{tag} {fam.name}: frame {f} (steps {int(steps[f])}) lane {lane}"


def decode(ctx, b, fam, max_sweeps=10, do_ml=1):
    out, sw, res, st = fam.buffers()
    ctx.decode(b.h, fam.sym, fam.era, max_sweeps=max_sweeps, do_ml=do_ml, out=out, sweeps=sw, residual=res, status=st)
    return out, sw, res, st


def keep(outs):
    return tuple(x.clone() for x in outs)


class Batch:
    pass


_CACHE = {}
_HANDLES = {}


def _plan_of(ctx, h, code, S):
    """The plan a decode at this S gets (one frame without erasures)."""
    z = torch.zeros((1, code.n, S), dtype=torch.uint8, device="cuda")
    ctx.decode(h, z, torch.zeros((1, code.n), dtype=torch.uint8, device="cuda"))
    ctx.synchronize()
    return ctx.last_plan()


def _codewords(ctx, h, code, F, S, seed):
    src = torch.randint(0, 256, (F, code.k, S), dtype=torch.uint8, device="cuda", generator=_gen(seed))
    return ctx.encode(h, src)


def _f1(ctx, b, ts_where, S, seed):
    """Parity-only frames: (t, where) per frame; even frames codewords, odd frames random bytes in every received symbol."""
    code = b.code
    F = len(ts_where)
    era = np.stack([sp.parity_subset(code, t, F1_SEED, w) for t, w in ts_where])
    cw = _codewords(ctx, b.h, code, F, S, seed)
    sym = cw.clone()
    sym[1::2] = torch.randint(0, 256, sym[1::2].shape, dtype=torch.uint8, device="cuda", generator=_gen(seed + 1))
    sym[_dev(era).bool()] = ERASED_FILL
    fam = Family("F1", sym, era, cw, [t for t, _ in ts_where])
    ref = _dev(sp.single_sweep_reference(code, sym.cpu().numpy(), era))
    even = torch.arange(0, F, 2, device="cuda")
    assert torch.equal(ref[even], cw[even])        # on codewords one sweep restores the codeword: reference and encoder agree
    i32 = lambda v: torch.full((F,), v, dtype=torch.int32, device="cuda")  # noqa: E731
    fam.want[(10, 1)] = dict(out=ref, good=None, lanes=(), sweeps=i32(1), residual=i32(0), status=i32(0))
    return fam


def _exact(ctx, b, name, Es, S, seed, pattern_seed, caps=((10, 1),)):
    """Exact-E frames on codewords; per (max_sweeps, do_ml) the oracle's numbers on the pattern."""
    code, oc = b.code, b.oc
    F = len(Es)
    era = np.stack([sp.exact_subset(code, E, pattern_seed) for E in Es])
    cw = _codewords(ctx, b.h, code, F, S, seed)
    sym = cw.clone()
    sym[_dev(era).bool()] = ERASED_FILL
    lane_host = {lane: np.ascontiguousarray(sym[:, :, lane].cpu().numpy()) for lane in (0, S - 1)}
    fam = Family(name, sym, era, cw, Es)
    for it, ml in caps:
        o0, sw, res, st = oc.decode_batch_s1(lane_host[0], era, itenum=it, do_ml=ml)
        good = np.isin(st, (0, 1))
        lanes = []
        for f in np.flatnonzero(~good):
            lanes.append((int(f), 0, _dev(o0[f])))
            lanes.append((int(f), S - 1, _dev(oc.decode_batch_s1(lane_host[S - 1][f:f + 1], era[f:f + 1], itenum=it, do_ml=ml)[0][0])))
        fam.want[(it, ml)] = dict(out=cw, good=_dev(good), lanes=lanes, sweeps=_dev(sw), residual=_dev(res), status=_dev(st),
                                  steps=np.asarray(Es) - res, status_host=st)
    fam.steps = fam.want[caps[0]]["steps"]
    return fam


def batch(ctx, oracle, name):
    """The batch `name`, built once: the code, its plan, its families."""
    if name in _CACHE:
        return _CACHE[name]
    ci, S, nthr, two, piece = BATCHES[name]
    if not codes.have_builtin(ci):
        pytest.skip(f"built-in code {ci} is not present")
    for k in KNOBS:
        ctx.configure(k, None)
    b = Batch()
    b.name, b.S = name, S
    b.code = codes.load_builtin(ci)
    if ci not in _HANDLES:
        _HANDLES[ci] = ctx.load_builtin_code(ci, codes.DEFAULT_COEF_SEED[ci])
    b.h = _HANDLES[ci]
    b.oc = oracle.OracleCode(b.code)
    b.plan = _plan_of(ctx, b.h, b.code, S)
    b.cap = b.plan["tier1_cap"]
    m, n = b.code.n - b.code.k, b.code.n
    edge = sorted({t for t in (b.cap - 1, b.cap, b.cap + 1, m - 1, m) if 0 <= t <= m})
    b.f1_rows = [(t, "random") for t in range(m + 1)] + [(t, w) for w in ("first", "last") for t in edge]
    b.f1 = _f1(ctx, b, b.f1_rows, S, seed=1000 + ci)
    two_tier = two == 1
    b.f2 = _exact(ctx, b, "F2", list(range(int(np.floor(0.18 * n)) + 1)), S, 2000 + ci, F2_SEED,
                  caps=((10, 1), (1, 1), (2, 1)) if two_tier else ((10, 1),))
    b.f3 = None
    if ci in (1, 3):
        b.f3 = _exact(ctx, b, "F3", list(range(int(np.ceil(0.19 * n)), int(np.floor(0.23 * n)) + 1, 2)), S, 3000 + ci, F3_SEED)
    _CACHE[name] = b
    return b


def limits(code, B, nslots):
    """The largest step counts at which the lists / the pull records still fit behind nslots accumulators of B bytes."""
    cdw = int(np.bincount(code.cols, minlength=code.n).max())
    return (nslots * B) // (B + 4 * cdw), (nslots * B - 16) // (B + 4 * cdw + 10)


# ------------------------------------------------------------------------------------------------ 1. the default plan
@pytest.mark.parametrize("name", list(BATCHES))
def test_default_plan_every_step_count(ctx, oracle, name):
    b = batch(ctx, oracle, name)
    ci, S, nthr, two, piece = BATCHES[name]
    m = b.code.n - b.code.k
    assert b.plan["two_tiers"] == two and b.plan["packet_bytes_per_workgroup"] == piece, b.plan
    assert (1 <= b.cap < m) if two else (b.cap == m)
    for fam in (b.f1, b.f2, b.f3):
        if fam is None:
            continue
        for key in fam.want:
            outs = decode(ctx, b, fam, *key)
            check_family(fam, outs, key, f"{name} default sweeps<={key[0]}")
            if key == (10, 1):
                fam.default = keep(outs)
    plan, names = ctx.last_plan(), ctx.profile_kernel_names()
    assert all(plan[key] == b.plan[key] for key in ("tier1_cap", "two_tiers", "packet_bytes_per_workgroup")), (plan, b.plan)
    lpr = piece // 16
    assert names["apply"].startswith(f"ldpc_scatter_kernel<{lpr},"), names       # LPR fixes the threads: 1024 / 512 / 256
    assert nthr == (1024 if lpr >= 8 else 512 if lpr >= 2 else 256)
    t1 = limits(b.code, piece, b.cap)
    t2 = limits(b.code, piece, m)
    print(f"{name}: tier1_cap {b.cap}, lists fit up to {t1[0]} steps in tier 1" +
          (f" and {t2[0]} in tier 2, pull records up to {t2[1]}" if two else "") + f"; swept 0..{m}")
    assert 0 < t1[0] < b.cap and (not two or b.cap < t2[1] < t2[0] < m)          # every limit lies inside the swept range
    if two:
        assert "ldpc_scatter_big_kernel" in names["apply_tier2"], names
        # (from the oracle's numbers) the ML stage writes back behind both tiers
        for fam in (b.f2,):
            st1 = np.zeros(2, dtype=bool)
            for key, w in fam.want.items():
                s1 = w["status_host"] == 1
                st1 |= [bool((s1 & (w["steps"] <= b.cap)).any()), bool((s1 & (w["steps"] > b.cap)).any())]
            assert st1.all(), (name, st1)


# ------------------------------------------------------------------------------------------------ 2. plan variants on A256
@pytest.mark.parametrize("knob,value", VARIANTS)
def test_plan_variants_give_the_default_bytes(ctx, oracle, knob, value):
    b = batch(ctx, oracle, "A256")
    for fam in (b.f1, b.f2):
        if fam.default is None:
            fam.default = keep(decode(ctx, b, fam))
            check_family(fam, fam.default, (10, 1), "A256 default")
    ctx.configure(knob, value)
    try:
        for fam in (b.f1, b.f2):
            outs = decode(ctx, b, fam)
            check_family(fam, outs, (10, 1), f"A256 {knob}={value}")
            for got, want, what in zip(outs, fam.default, ("bytes", "sweeps", "residual", "status")):
                assert_same(got, want, fam.steps, f"A256 {knob}={value} {fam.name} {what} against the default run")
        plan = ctx.last_plan()
        print(f"A256 {knob}={value}: tier1_cap {plan['tier1_cap']} two_tiers {plan['two_tiers']} piece {plan['packet_bytes_per_workgroup']}")
        assert 0 <= plan["tier1_cap"] <= b.code.n - b.code.k
    finally:
        ctx.configure(knob, None)
    assert ctx.knobs() == ""


# ------------------------------------------------------------------------------------------------ 3. tier-2 pieces and rows in flight
def _wide(ctx, oracle):
    """An S = 1024 copy of A256 (SCATTER_T2P needs several slices per row), restricted to the step counts around tier1_cap, around
    the two LDS-fit limits of tier 2 and at the end, plus the heavy frames."""
    if "wide" in _CACHE:
        return _CACHE["wide"]
    a = batch(ctx, oracle, "A256")
    b = Batch()
    b.name, b.S, b.code, b.h, b.oc = "A1024", 1024, a.code, a.h, a.oc
    b.plan = _plan_of(ctx, b.h, b.code, 1024)
    b.cap = b.plan["tier1_cap"]
    m = b.code.n - b.code.k
    lists, pulls = limits(b.code, 256, m)
    ts = sorted(set(range(b.cap - 2, b.cap + 3)) | set(range(430, 461)) | set(range(lists - 2, lists + 3)) | set(range(506, 511)))
    assert pulls in ts and lists in ts and ts[-1] == m
    b.f1 = _f1(ctx, b, [(t, "random") for t in ts], 1024, seed=4001)
    n = b.code.n
    b.f3 = _exact(ctx, b, "F3", list(range(int(np.ceil(0.19 * n)), int(np.floor(0.23 * n)) + 1, 2)), 1024, 4003, F3_SEED)
    _CACHE["wide"] = b
    return b


@pytest.mark.parametrize("knob,value", [(None, None), ("SCATTER_T2P", "1"), ("SCATTER_T2P", "2"), ("SCATTER_T2P", "4"),
                                        ("SCATTER_R2", "2"), ("SCATTER_R2", "4")])
def test_tier2_pieces_and_rows_in_flight(ctx, oracle, knob, value):
    b = _wide(ctx, oracle)
    assert b.plan["two_tiers"] == 1 and b.plan["packet_bytes_per_workgroup"] == 256
    for fam in (b.f1, b.f3):
        if fam.default is None:
            fam.default = keep(decode(ctx, b, fam))
    if knob:
        ctx.configure(knob, value)
    try:
        for fam in (b.f1, b.f3):
            outs = decode(ctx, b, fam)
            check_family(fam, outs, (10, 1), f"A1024 {knob}={value}")
            for got, want, what in zip(outs, fam.default, ("bytes", "sweeps", "residual", "status")):
                assert_same(got, want, fam.steps, f"A1024 {knob}={value} {fam.name} {what} against the default run")
        assert "ldpc_scatter_big_kernel" in ctx.profile_kernel_names()["apply_tier2"]
    finally:
        if knob:
            ctx.configure(knob, None)


# ------------------------------------------------------------------------------------------------ 4. the large code without pairs / relaxation
@pytest.mark.parametrize("knob,value", [("SCATTER_PAIRS", "0"), ("PEEL_RELAX", "0")])
def test_large_code_variants(ctx, oracle, knob, value):
    b = batch(ctx, oracle, "C128")
    ctx.configure(knob, value)
    try:
        for fam in (b.f1, b.f2, b.f3):
            outs = decode(ctx, b, fam)
            check_family(fam, outs, (10, 1), f"C128 {knob}={value}")
            if fam.default is not None:
                for got, want, what in zip(outs, fam.default, ("bytes", "sweeps", "residual", "status")):
                    assert_same(got, want, fam.steps, f"C128 {knob}={value} {fam.name} {what} against the default run")
        assert ctx.last_plan()["two_tiers"] == 1
    finally:
        ctx.configure(knob, None)


# ------------------------------------------------------------------------------------------------ 5. entry points
def test_in_place(ctx, oracle):
    b = batch(ctx, oracle, "A256")
    fam = b.f1
    sym = fam.sym.clone()
    _, sw, res, st = fam.buffers()
    out, sw, res, st = ctx.decode(b.h, sym, fam.era, sweeps=sw, residual=res, status=st, inplace=True)
    assert out.data_ptr() == sym.data_ptr()
    check_family(fam, (out, sw, res, st), (10, 1), "A256 in place")
    assert ctx.profile_kernel_names()["apply"].endswith("true>")                   # the INPLACE instantiation


def test_decode_frames(ctx, oracle):
    b = batch(ctx, oracle, "A256")
    fam = b.f1
    F, n, S = fam.sym.shape
    out, sw, res, st = fam.buffers()
    eo = torch.full((F, n), POISON, dtype=torch.uint8, device="cuda")
    rsrc = torch.full((F,), POISON32, dtype=torch.int32, device="cuda")
    rc = ctx._L.ldpc_amd_decode_frames(ctx._h, b.h, S, F, fam.sym.data_ptr(), fam.era.data_ptr(), 10, 1, out.data_ptr(), sw.data_ptr(),
                                       res.data_ptr(), st.data_ptr(), eo.data_ptr(), rsrc.data_ptr(), api.DEVICE_PTRS)
    assert rc == 0, ctx._L.ldpc_amd_last_error(ctx._h)
    check_family(fam, (out, sw, res, st), (10, 1), "A256 decode_frames")
    assert_same(eo, torch.zeros_like(eo), fam.steps, "A256 decode_frames erased_out")
    assert_same(rsrc, torch.zeros_like(rsrc), fam.steps, "A256 decode_frames residual_src")


class RxBuffers:
    def __init__(self, nb, n, S):
        self.out = torch.empty((nb, n, S), dtype=torch.uint8, device="cuda")
        self.i32 = [torch.empty((nb,), dtype=torch.int32, device="cuda") for _ in range(4)]    # sweeps residual status residual_src
        self.eo = torch.empty((nb, n), dtype=torch.uint8, device="cuda")

    def poison(self):
        self.out.fill_(POISON)
        self.eo.fill_(POISON)
        for t in self.i32:
            t.fill_(POISON32)

    def take(self, nb):
        return [self.out[:nb].clone(), self.i32[0][:nb].clone(), self.i32[1][:nb].clone(), self.i32[2][:nb].clone(), self.eo[:nb].clone(),
                self.i32[3][:nb].clone()]


def _receive(ctx, b, pk, counts, closable):
    """The stream pk (frames in order, counts[f] packets of frame f) through FecRxDevice: decode_many in calls of up to 64 blocks for
    the frames the receiver's close rule closes, decode_flush for those it cannot close (fewer than k + round(0.2 m) + 1 symbols
    arrive: such a block ends only with the stream).  Returns (block numbers, the six outputs of all frames in order, seen)."""
    import ctypes as C
    code, S = b.code, b.S
    n = code.n
    rx = ctx.fec_rx_device(n, code.k, S)
    many, one = RxBuffers(64, n, S), RxBuffers(1, n, S)
    off = np.concatenate([[0], np.cumsum(counts)])
    blocks, parts, seen = [], [], {}

    def feed(p0, p1):
        while p0 < p1:
            many.poison()
            bl = np.zeros(64, dtype=np.int32)
            used = C.c_int64(0)
            nb = ctx._check(ctx._L.ldpc_amd_fec_rx_dev_decode_many(
                rx._h, b.h, pk[p0:p1].data_ptr(), p1 - p0, 10, 1, many.out.data_ptr(), many.i32[0].data_ptr(), many.i32[1].data_ptr(),
                many.i32[2].data_ptr(), many.eo.data_ptr(), many.i32[3].data_ptr(), bl.ctypes.data, 64, C.byref(used)), "decode_many")
            assert used.value > 0
            if nb:
                blocks.extend(bl[:nb].tolist())
                parts.append(many.take(nb))
                names = ctx.profile_kernel_names()     # (read here: a flush is a one-frame decode from an array of rows)
                seen.setdefault("caps", set()).add((ctx.last_plan()["tier1_cap"], ctx.last_plan()["two_tiers"]))
                seen.setdefault("apply", set()).add(names["apply"])
                seen.setdefault("tier2", set()).add(names["apply_tier2"])
                seen.setdefault("paths", set()).add(ctx.fec_receiver_info()["path"])
            p0 += used.value

    def flush():
        one.poison()
        blk = C.c_int(-1)
        rc = ctx._check(ctx._L.ldpc_amd_fec_rx_dev_decode_flush(
            rx._h, b.h, 10, 1, one.out.data_ptr(), one.i32[0].data_ptr(), one.i32[1].data_ptr(), one.i32[2].data_ptr(), one.eo.data_ptr(),
            one.i32[3].data_ptr(), C.byref(blk)), "decode_flush")
        if rc == 1:
            blocks.append(blk.value)
            parts.append(one.take(1))
        return rc

    try:
        F, f = len(counts), 0
        while f < F:
            if closable[f]:
                g = f
                while g < F and closable[g] and g - f < 64:
                    g += 1
                feed(int(off[f]), int(off[g]))
                f = g
            else:
                feed(int(off[f]), int(off[f + 1]))      # (its first packets close the block before it)
                assert flush() == 1
                f += 1
        while flush() == 1:
            pass
        assert rx.dropped == 0
    finally:
        ctx.synchronize()
        rx.close()
    return np.array(blocks), [torch.cat(x) for x in zip(*parts)], seen


@pytest.mark.parametrize("dyn", [None, "2"])
def test_fused_receiver(ctx, oracle, dyn):
    """Only codewords go through the wire: the frames of F1 as codewords, the packets of the erased symbols dropped."""
    b = batch(ctx, oracle, "A256")
    fam = b.f1
    code, S = b.code, b.S
    n, k, m = code.n, code.k, code.n - code.k
    F = fam.F
    pk = ctx.fec_packetize_device(fam.cw, 1, 0)
    pk = pk[~fam.era.reshape(-1).bool()].contiguous()          # exactly the flagged packets are lost, nothing is re-ordered
    counts = n - fam.era_host.sum(1).astype(np.int64)
    assert pk.shape[0] == counts.sum()
    closable = counts > k + int(round(0.2 * m))                 # the close rule of include/ldpc_erasure_amd_wire.h
    if dyn:
        ctx.configure("SCATTER_DYN", dyn)
    try:
        blocks, got, seen = _receive(ctx, b, pk, counts, closable)
    finally:
        if dyn:
            ctx.configure("SCATTER_DYN", None)
    assert np.array_equal(blocks, np.arange(F) & 0xFF)
    out, sw, res, st, eo, rsrc = got
    assert_same(out, fam.cw, fam.steps, f"receiver DYN={dyn} bytes")
    for t, v, what in ((sw, 1, "sweeps"), (res, 0, "residual"), (st, 0, "status"), (rsrc, 0, "residual_src")):
        assert_same(t, torch.full_like(t, v), fam.steps, f"receiver DYN={dyn} {what}")
    assert_same(eo, torch.zeros_like(eo), fam.steps, f"receiver DYN={dyn} erased_out")
    assert seen["paths"] == {"fused"}, seen["paths"]
    assert all(a.startswith("ldpc_scatter_pktin_kernel<") for a in seen["apply"]), seen["apply"]
    assert any(a.startswith("ldpc_scatter_pktin_big_kernel<") for a in seen["tier2"]), seen["tier2"]
    assert len(seen["caps"]) == 1, seen["caps"]
    cap, two = next(iter(seen["caps"]))
    print(f"A256 packets-in DYN={dyn}: tier1_cap {cap} (array plan: {b.cap})")
    assert two == 1 and cap < b.cap                                     # the row-source words cost tier 1 accumulators
    _CACHE.setdefault("pin_caps", {})[dyn] = cap
    if dyn and None in _CACHE["pin_caps"]:
        assert cap < _CACHE["pin_caps"][None]                           # ... and the list of received rows costs some more
    # frames on both sides of, and on, the packets-in cap went through the packets-in kernels
    assert {cap - 1, cap, cap + 1} <= set(np.asarray(fam.steps)[closable].tolist())


# ------------------------------------------------------------------------------------------------ 6. ragged order
def test_ragged_order(ctx, oracle):
    """The frames of A256 -- F1 interleaved with F2 and F3 -- in a seeded random permutation: the frames of tier 2 are then neither
    sorted nor contiguous in the batch, and every frame must still get its own bytes."""
    b = batch(ctx, oracle, "A256")
    fams = (b.f1, b.f2, b.f3)
    for fam in fams:
        if fam.default is None:
            fam.default = keep(decode(ctx, b, fam))
            check_family(fam, fam.default, (10, 1), "A256 default")
    perm = torch.from_numpy(np.random.default_rng(6).permutation(sum(f.F for f in fams))).cuda()
    sym = torch.cat([f.sym for f in fams])[perm].contiguous()
    era = torch.cat([f.era for f in fams])[perm].contiguous()
    steps = np.concatenate([f.steps for f in fams])[perm.cpu().numpy()]
    F = sym.shape[0]
    out = torch.full_like(sym, POISON)
    sw, res, st = (torch.full((F,), POISON32, dtype=torch.int32, device="cuda") for _ in range(3))
    ctx.decode(b.h, sym, era, out=out, sweeps=sw, residual=res, status=st)
    for i, (got, what) in enumerate(zip((out, sw, res, st), ("bytes", "sweeps", "residual", "status"))):
        want = torch.cat([f.default[i] for f in fams])[perm]
        assert_same(got, want, steps, f"A256 ragged {what}")
    assert ctx.last_plan()["two_tiers"] == 1
