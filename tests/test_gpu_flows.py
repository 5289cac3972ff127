"""GPU tests of the multi-flow receiver (include/ldpc_erasure_amd_flows.h): many FEC streams reassembled and decoded per call.

The expected values are built WITHOUT the code under test: one host reassembler api.FecRx per flow, fed the flow's segments with
the same call boundaries (tools/flow_streams.py), gives closes, blocks, consumed and dropped counts and the received symbols and
flags; the CPU oracle gives the decoded frames (test_gpu_receiver.oracle_frames).  What the streams exercise is asserted without a
GPU in tests/test_flow_streams_cpu.py.  On top of that: which path ran, tier 2 and the ML stage behind the packets-in kernels, the
composed paths, equality with separate FecRxDevice objects and with any mix of push_many and decode_many, more flows than a
wavefront has lanes, word-sized symbols, guard bands around every output, and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ldpc_erasure_codes_amd import api, codes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_receiver import oracle_frames, random_code, same_frames, to_host  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flow_streams as fs  # noqa: E402

EINVAL, ENOMEM, ENOCODE, EUNSUP = -1, -3, -4, -5
MIB = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


_CODES = {}


def get_code(ctx, which):
    """(handle, codes.Code) of built-in code `which` or the random (300,200) code ("rand"), registered once with THIS module's
    context (test_gpu_receiver.get_code keeps the handles of its own context)."""
    if which not in _CODES:
        if which == "rand":
            code = random_code()
            _CODES[which] = (ctx.register_code(code), code)
        else:
            _CODES[which] = (ctx.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which]), codes.load_builtin(which))
    return _CODES[which]


def to_dev(a, offset=0):
    """The array on the device, its first byte `offset` bytes behind a 256-byte boundary."""
    buf = torch.zeros(a.size + 256, dtype=torch.uint8, device="cuda")
    v = buf[offset:offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert a.size == 0 or v.data_ptr() % 256 == offset
    return v


def collect(ctx, h, code, S, sc, pick=lambda i: True, it=10, do_ml=1, offset=0, seen=None, after=None):
    """The stream set through ONE flows object over the reference run's call boundaries: call i through decode_many if pick(i), else
    through push_many + decode_frames.  Returns what every call and every flush returned, on the host."""
    nf = len(sc["flows"])
    rx = ctx.fec_rx_flows(nf, code.n, code.k, S)
    res = []
    for i, call in enumerate(sc["calls"]):
        pk_host, fb = fs.call_packets(sc["flows"], call)
        pk = to_dev(pk_host, offset)
        if pick(i):
            closes, blocks, fr, consumed = rx.decode_many(h, pk, fb, call["mb"], max_sweeps=it, do_ml=do_ml)
        else:
            closes, blocks, sym, er, consumed = rx.push_many(pk, fb, call["mb"])
            fr = ctx.decode_frames(h, sym[:, :, 0].contiguous() if S == 1 else sym, er, max_sweeps=it, do_ml=do_ml) if len(blocks) else None
        ctx.synchronize()
        r = dict(closes=closes, blocks=blocks, consumed=consumed, dropped=rx.dropped, frames=to_host(fr, S) if len(blocks) else None)
        if pick(i) and len(blocks):
            r["info"] = ctx.fec_receiver_info()
            if seen is not None:
                seen.update(plan=ctx.last_plan(), names=ctx.profile_kernel_names(), info=r["info"])
        res.append(r)
        if after is not None:
            after(i, rx)
    flushes = []
    for f in range(nf):
        fl = []
        while True:
            r = rx.decode_flush(f, h, max_sweeps=it, do_ml=do_ml)
            if r is None:
                break
            ctx.synchronize()
            fl.append((r[0], to_host(r[1], S)))
        flushes.append(fl)
    dropped = rx.dropped
    rx.close()
    return res, flushes, dropped


def wants(sc, oc, code, S, it, do_ml):
    """The oracle's frames of every call and flush of the reference run (computed once per stream set and decoder setting)."""
    key = ("want", it, do_ml)
    if key not in sc:
        per_call = []
        for call in sc["calls"]:
            e = fs.expected(call, code.n, S)
            per_call.append(oracle_frames(oc, code, e["sym"], e["er"], it, do_ml) if len(e["blocks"]) else None)
        per_flush = [[oracle_frames(oc, code, sym[None], er[None], it, do_ml) for _, sym, er in fl] for fl in sc["flushes"]]
        sc[key] = (per_call, per_flush)
    return sc[key]


def check(got, sc, oc, code, S, it=10, do_ml=1, path=None):
    """Every call and flush of `got` (collect) against the host receivers and the oracle."""
    res, flushes, _ = got
    per_call, per_flush = wants(sc, oc, code, S, it, do_ml)
    assert len(res) == len(sc["calls"])
    for i, (r, call) in enumerate(zip(res, sc["calls"])):
        e = fs.expected(call, code.n, S)
        for name in ("closes", "blocks", "consumed", "dropped"):
            assert r[name].dtype == e[name].dtype and np.array_equal(r[name], e[name]), (i, name, r[name], e[name])
        if len(e["blocks"]):
            same_frames(r["frames"], per_call[i], (i, call["mb"]))
            if path is not None and "info" in r:
                assert r["info"]["path"] == path and r["info"]["blocks"] == len(e["blocks"]), (i, r["info"])
    for f, (fl, ref) in enumerate(zip(flushes, sc["flushes"])):
        assert [b for b, _ in fl] == [b for b, _, _ in ref], f
        for j, (_, fr) in enumerate(fl):
            same_frames(fr, per_flush[f][j], ("flush", f, j))


def same_runs(a, b, tag):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        for name in ("closes", "blocks", "consumed", "dropped"):
            assert np.array_equal(x[name], y[name]), (tag, i, name)
        assert (x["frames"] is None) == (y["frames"] is None)
        if x["frames"] is not None:
            same_frames(x["frames"], y["frames"], (tag, i))
    assert len(a[0]) == len(b[0]) and len(a[1]) == len(b[1])
    for f, (fa, fb) in enumerate(zip(a[1], b[1])):
        assert [x[0] for x in fa] == [x[0] for x in fb], (tag, f)
        for (_, x), (_, y) in zip(fa, fb):
            same_frames(x, y, (tag, "flush", f))
    assert np.array_equal(a[2], b[2]), tag


# ---------------------------------------------------------------------------------------------- 1. bytes against host receivers + oracle
@pytest.mark.parametrize("S", [16, 128])
def test_flows_equal_host_receivers_and_oracle(ctx, oracle, S):
    h, code = get_code(ctx, "rand")
    oc = oracle.OracleCode(code)
    sc = fs.scenario("mixed", oc, code, S)
    assert sum(fs.closed_per_flow(sc)) >= sum(sc["F"]) - 6
    got = collect(ctx, h, code, S, sc)
    check(got, sc, oc, code, S, path="fused")
    assert (got[0][-1]["dropped"] > 0).any() and got[0][-1]["dropped"][0] == 0


# ---------------------------------------------------------------------------------------------- 2. the built-in code, tier 2 and the ML stage
@pytest.mark.parametrize("S", [1024, 128])
def test_builtin_code_fused_with_tier2_and_ml_stage(ctx, oracle, S):
    h, code = get_code(ctx, 1)
    oc = oracle.OracleCode(code)
    sc = fs.scenario("builtin", oc, code, S)
    seen = {}
    got = collect(ctx, h, code, S, sc, it=1, seen=seen)    # one sweep leaves the 20 % flow's frames to tier 2 and the ML stage
    check(got, sc, oc, code, S, it=1, path="fused")
    per_call, per_flush = wants(sc, oc, code, S, 1, 1)
    status = np.concatenate([w.status for w in per_call if w is not None])
    assert (status == 1).any()                              # ... which solves them
    lost = np.concatenate([fs.expected(c, code.n, S)["er"] for c in sc["calls"]]).sum(1)
    plan, names = seen["plan"], seen["names"]
    assert names["apply"].startswith("ldpc_scatter_pktin_kernel<")
    # A block closes only with more than k + 0.2 (n - k) = 1632 packets, so a receiver hands the decoder at most 407 erasures.  Tier 1
    # of the S = 1024 plan takes fewer than that, tier 1 of the S = 128 plan more: only at S = 1024 can a received block reach tier 2.
    assert plan["two_tiers"] == 1 and (lost < plan["tier1_cap"]).any()
    assert plan["tier1_cap"] >= code.n - fs.min_parity_rx(code.n, code.k) or S == 1024
    if S == 1024:
        assert (lost > plan["tier1_cap"]).any() and names["apply_tier2"].startswith("ldpc_scatter_pktin_big_kernel<")


# ---------------------------------------------------------------------------------------------- 3. the composed paths
def test_composed_paths_give_the_same_bytes(oracle):
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        from test_gpu_sender import heavy_code
        code, hv = random_code(), heavy_code()
        h, hh = c.register_code(code), c.register_code(hv)
        oc = oracle.OracleCode(code)
        sc1 = fs.scenario("mixed", oc, code, 1)
        check(collect(c, h, code, 1, sc1), sc1, oc, code, 1, path="composed")          # S = 1
        sc = fs.scenario("mixed", oc, code, 16)
        c.configure("LDPC_AMD_RX_PKT", 0)
        check(collect(c, h, code, 16, sc), sc, oc, code, 16, path="composed")          # the knob
        c.configure("LDPC_AMD_RX_PKT", None)
        check(collect(c, h, code, 16, sc, offset=4), sc, oc, code, 16, path="composed")   # packets 4 bytes off 8-byte alignment
        check(collect(c, h, code, 16, sc), sc, oc, code, 16, path="fused")
        ohv = oracle.OracleCode(hv)
        sch = fs.scenario("heavy", ohv, hv, 128)
        check(collect(c, hh, hv, 128, sch), sch, ohv, hv, 128, path="composed")        # column degrees above 16
        assert 0 < c.fec_receiver_info()["scratch_bytes"] <= 256 * MIB


# ---------------------------------------------------------------------------------------------- 4. equivalence with separate receivers
def collect_separate(ctx, h, code, S, sc):
    """The same calls through one FecRxDevice per flow."""
    nf = len(sc["flows"])
    rxs = [ctx.fec_rx_device(code.n, code.k, S) for _ in range(nf)]
    res = []
    for call in sc["calls"]:
        per = []
        for f, cf in enumerate(call["flows"]):
            b, fr, used = rxs[f].decode_many(h, to_dev(sc["flows"][f][cf["pos"]:cf["pos"] + cf["c"]]), call["mb"])
            ctx.synchronize()
            per.append((b, to_host(fr, S) if len(b) else None, used))
        blocks = np.concatenate([p[0] for p in per]).astype(np.int32)
        frames = [p[1] for p in per if p[1] is not None]
        res.append(dict(closes=np.array([len(p[0]) for p in per], dtype=np.int32), blocks=blocks,
                        consumed=np.array([p[2] for p in per], dtype=np.int64), dropped=np.array([r.dropped for r in rxs], dtype=np.int64),
                        frames=api.DecodedFrames(*[np.concatenate(x) for x in zip(*frames)]) if frames else None))
    flushes = []
    for rx in rxs:
        fl = []
        while True:
            r = rx.decode_flush(h)
            if r is None:
                break
            ctx.synchronize()
            fl.append((r[0], to_host(r[1], S)))
        flushes.append(fl)
    dropped = np.array([r.dropped for r in rxs], dtype=np.int64)
    for rx in rxs:
        rx.close()
    return res, flushes, dropped


def test_equivalence_with_separate_receivers_and_any_mix_of_calls(ctx, oracle):
    h, code = get_code(ctx, "rand")
    oc = oracle.OracleCode(code)
    S = 16
    sc = fs.scenario("mixed", oc, code, S)
    ref = collect(ctx, h, code, S, sc)
    same_runs(ref, collect_separate(ctx, h, code, S, sc), "separate FecRxDevice objects")
    rng = np.random.default_rng(4)
    coin = rng.integers(0, 2, size=len(sc["calls"]))
    for name, pick in (("push_many + decode_frames", lambda i: False), ("alternating", lambda i: i % 2 == 0), ("random", lambda i: bool(coin[i]))):
        same_runs(ref, collect(ctx, h, code, S, sc, pick=pick), name)
    # nflows = 1: the object is a FecRxDevice
    one = dict(flows=sc["flows"][4:], calls=[dict(mb=c["mb"], flows=c["flows"][4:]) for c in sc["calls"]], flushes=sc["flushes"][4:])
    same_runs(collect(ctx, h, code, S, one), collect_separate(ctx, h, code, S, one), "nflows = 1")


# ---------------------------------------------------------------------------------------------- 5. more flows than lanes
def test_many_flows_in_one_call(ctx, oracle):
    h, code = get_code(ctx, "rand")
    oc = oracle.OracleCode(code)
    sc = fs.scenario("many", oc, code, 16)
    assert len(sc["flows"]) == 130 and len(sc["calls"]) == 1
    closes = fs.expected(sc["calls"][0], code.n, 16)["closes"]
    assert closes.sum() > 130 and len(set(closes.tolist())) > 1       # slot bases are not a multiple of anything
    check(collect(ctx, h, code, 16, sc), sc, oc, code, 16, path="fused")


# ---------------------------------------------------------------------------------------------- 6. word-sized symbols
def test_word_sized_symbols(oracle):
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.set_symbol_unit(4)
        code = random_code()
        h = c.register_code(code)
        oc = oracle.OracleCode(code)
        sc = fs.scenario("words", oc, code, 20)
        got = collect(c, h, code, 20, sc)
        check(got, sc, oc, code, 20, path="fused")
        pad = []
        for pk in sc["flows"]:                                           # the same streams, every payload zero-padded to 32 bytes
            p = np.zeros((pk.shape[0], 8 + 32), dtype=np.uint8)
            p[:, :28] = pk
            pad.append(p)
        got32 = collect(c, h, code, 32, dict(flows=pad, calls=sc["calls"], flushes=sc["flushes"]))

        def cut(fr):
            assert not fr.out[:, :, 20:].any()
            return fr._replace(out=np.ascontiguousarray(fr.out[:, :, :20]))
        res32 = [dict(r, frames=cut(r["frames"]) if r["frames"] is not None else None) for r in got32[0]]
        same_runs(got, (res32, [[(b, cut(fr)) for b, fr in fl] for fl in got32[1]], got32[2]), "zero-padded S = 32")


# ---------------------------------------------------------------------------------------------- 7. guard bands
@pytest.mark.parametrize("knob", [None, 0])
def test_guard_bands_and_untouched_slots(ctx, oracle, knob):
    h, code = get_code(ctx, "rand")
    n, k, S, nf, MB, G = code.n, code.k, 16, 3, 8, 4096
    flows = [f[0] for f in fs.equal_flows(oracle.OracleCode(code), code, S, nf, 5, 6000)]
    pk_host, fb = fs.flow_begin_of(flows)
    pk = to_dev(pk_host)
    before = pk.clone()
    slots = nf * MB
    L = ctx._L
    sizes = dict(out=slots * n * S, sweeps=4 * slots, residual=4 * slots, status=4 * slots, erased_out=slots * n, residual_src=4 * slots,
                 sym=slots * n * S, er=slots * n)
    bufs = {kk: torch.full((v + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda") for kk, v in sizes.items()}
    ptr = {kk: bufs[kk].data_ptr() + G for kk in bufs}
    blocks = np.full(slots + 2, -7, dtype=np.int32)
    closes = np.full(nf + 2, -7, dtype=np.int32)
    used = np.full(nf + 2, -7, dtype=np.int64)
    ctx.configure("LDPC_AMD_RX_PKT", knob)
    try:
        with ctx.fec_rx_flows(nf, n, k, S) as rx:
            T = L.ldpc_amd_fec_rx_flows_decode_many(rx._h, h, pk.data_ptr(), fb.ctypes.data, 10, 1, ptr["out"], ptr["sweeps"], ptr["residual"],
                                                    ptr["status"], ptr["erased_out"], ptr["residual_src"], blocks[1:].ctypes.data,
                                                    closes[1:].ctypes.data, MB, used[1:].ctypes.data)
            ctx.synchronize()
        with ctx.fec_rx_flows(nf, n, k, S) as rx:
            T2 = L.ldpc_amd_fec_rx_flows_push_many(rx._h, pk.data_ptr(), fb.ctypes.data, ptr["sym"], ptr["er"], None, None, MB, None)
            ctx.synchronize()
    finally:
        ctx.configure("LDPC_AMD_RX_PKT", None)
    assert nf * 2 <= T < slots and T2 == T and closes[1:1 + nf].sum() == T and np.array_equal(used[1:1 + nf], np.diff(fb))
    assert closes[0] == -7 and (closes[1 + nf:] == -7).all() and used[0] == -7 and (used[1 + nf:] == -7).all()
    assert blocks[0] == -7 and (blocks[1 + T:] == -7).all() and (blocks[1:1 + T] >= 0).all()
    assert torch.equal(pk, before)                           # the packet array is only read
    for kk, v in sizes.items():
        per = v // slots
        host = bufs[kk].cpu().numpy()
        assert (host[:G] == 0xA5).all() and (host[G + v:] == 0xA5).all(), kk
        assert (host[G + T * per:G + v] == 0xA5).all(), f"{kk}: slots at or beyond the total were touched"
        assert not (host[G:G + T * per] == 0xA5).all(), kk


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_leave_every_flow_where_it_was(ctx, oracle):
    L = ctx._L
    h, code = get_code(ctx, "rand")
    hb, _ = get_code(ctx, 1)
    n, k, S = code.n, code.k, 16
    oc = oracle.OracleCode(code)
    sc = fs.scenario("mixed", oc, code, S)
    nf = len(sc["flows"])
    MB = 4
    slots = nf * MB
    out = torch.full((slots, n, S), 0xA5, dtype=torch.uint8, device="cuda")
    er = torch.full((slots, n), 0xA5, dtype=torch.uint8, device="cuda")
    i32 = torch.zeros((4, slots), dtype=torch.int32, device="cuda")
    out_host = np.zeros((slots, n, S), dtype=np.uint8)
    seg = [pk[:40] for pk in sc["flows"]]
    pk_host, fb = fs.flow_begin_of(seg)
    pk = to_dev(pk_host)

    def refused(rc, want, text=None):
        assert rc == want, rc
        msg = L.ldpc_amd_last_error(ctx._h)
        assert msg and (text is None or text in msg), msg

    def fbs(*v):
        return np.array(v, dtype=np.int64)

    def after(i, rx):
        if i != 2:
            return
        state = rx.dropped.copy()

        def dec(code_h=h, packets=pk.data_ptr(), fb_=fb, it=10, out_p=out.data_ptr(), mb=MB):
            return L.ldpc_amd_fec_rx_flows_decode_many(rx._h, code_h, packets, fb_.ctypes.data if fb_ is not None else None, it, 1, out_p,
                                                       i32[0].data_ptr(), i32[1].data_ptr(), i32[2].data_ptr(), er.data_ptr(), i32[3].data_ptr(),
                                                       None, None, mb, None)

        def push(packets=pk.data_ptr(), fb_=fb, sym_p=out.data_ptr(), mb=MB):
            return L.ldpc_amd_fec_rx_flows_push_many(rx._h, packets, fb_.ctypes.data if fb_ is not None else None, sym_p, er.data_ptr(), None, None,
                                                     mb, None)

        for call in (dec, push):
            refused(call(fb_=None), EINVAL, b"flow_begin")
            refused(call(fb_=fb + 1), EINVAL, b"start at 0")
            bad = fb.copy()
            bad[2] = bad[3] + 1
            refused(call(fb_=bad), EINVAL, b"decreases")
            refused(call(fb_=fbs(0, 0, 0, 0, 1 << 30, 1 << 31)), EINVAL, b"2^31")
            refused(call(mb=0), EINVAL, b"max_blocks_per_flow")
            refused(call(mb=(1 << 31) // (nf * n) + 1), EINVAL, b"2^31 - 2")
            refused(call(packets=pk_host.ctypes.data), EINVAL, b"device pointer")
        refused(push(sym_p=out_host.ctypes.data), EINVAL, b"device pointers")
        refused(dec(out_p=out_host.ctypes.data), EINVAL, b"device pointers")
        refused(dec(code_h=hb), EINVAL, b"(2040,1530)")
        refused(dec(code_h=999), ENOCODE, b"unknown code handle")
        refused(dec(it=0), EINVAL, b"max_sweeps must be >= 1")
        for flow in (-1, nf):
            refused(L.ldpc_amd_fec_rx_flows_flush(rx._h, flow, out.data_ptr(), er.data_ptr(), None), EINVAL, b"no flow")
            refused(L.ldpc_amd_fec_rx_flows_decode_flush(rx._h, flow, h, 10, 1, out.data_ptr(), None, None, None, None, None, None), EINVAL, b"no flow")
            assert L.ldpc_amd_fec_rx_flows_dropped(rx._h, flow) == -1
        refused(L.ldpc_amd_fec_rx_flows_decode_flush(rx._h, 4, h, 0, 1, out.data_ptr(), None, None, None, None, None, None), EINVAL, b"max_sweeps")
        refused(L.ldpc_amd_fec_rx_flows_decode_flush(rx._h, 4, hb, 10, 1, out.data_ptr(), None, None, None, None, None, None), EINVAL, b"(2040,1530)")
        # P == 0: returns 0, nothing is touched (not even looked at: null pointers pass in decode_many)
        zero = np.zeros(nf + 1, dtype=np.int64)
        cl, us = np.full(nf, -7, dtype=np.int32), np.full(nf, -7, dtype=np.int64)
        assert L.ldpc_amd_fec_rx_flows_decode_many(rx._h, h, None, zero.ctypes.data, 10, 1, None, None, None, None, None, None, None,
                                                   cl.ctypes.data, MB, us.ctypes.data) == 0
        assert (cl == 0).all() and (us == 0).all()
        assert push(packets=None, fb_=zero) == 0
        ctx.synchronize()
        assert bool((out == 0xA5).all()) and bool((er == 0xA5).all()) and np.array_equal(rx.dropped, state)

    # creation
    hnd = C.c_void_p()
    for bad_nf in (0, -1, 4097):
        refused(L.ldpc_amd_fec_rx_flows_create(ctx._h, bad_nf, n, k, S, C.byref(hnd)), EINVAL, b"nflows")
    refused(L.ldpc_amd_fec_rx_flows_create(ctx._h, nf, n, n, S, C.byref(hnd)), EINVAL, b"0 < k < n")
    refused(L.ldpc_amd_fec_rx_flows_create(ctx._h, nf, n, k, S, None), EINVAL)
    refused(L.ldpc_amd_fec_rx_flows_create(ctx._h, 4096, 65536, 32768, 4096, C.byref(hnd)), ENOMEM)   # 2 TiB of staging planes
    # the decoder's own refusal: S = 24 with symbol unit 16
    with ctx.fec_rx_flows(2, n, k, 24) as rx24:
        pk24 = torch.zeros((50, 8 + 24), dtype=torch.uint8, device="cuda")
        fb24 = fbs(0, 20, 50)
        refused(L.ldpc_amd_fec_rx_flows_decode_many(rx24._h, h, pk24.data_ptr(), fb24.ctypes.data, 10, 1, out.data_ptr(), None, None, None, None,
                                                    None, None, None, 2, None), EUNSUP, b"S must be 1 or a multiple of 16 (got 24)")
        refused(L.ldpc_amd_fec_rx_flows_decode_flush(rx24._h, 0, h, 10, 1, out.data_ptr(), None, None, None, None, None, None), EUNSUP, b"multiple of 16")
    # every refusal in the middle of the stream: the calls before and behind it return the reference's values
    check(collect(ctx, h, code, S, sc, after=after), sc, oc, code, S, path="fused")
