"""GPU tests of the mixed calls of the multi-flow receiver (include/ldpc_erasure_amd_flows_mixed.h): packets of many flows in ONE
array in arrival order, a flow number per packet.

The expected values are built WITHOUT the code under test.  The partition alone is checked against np.argsort(kind="stable") and
np.bincount.  The receiver is checked as tests/test_gpu_flows.py checks the segmented calls: one host reassembler api.FecRx per flow
over the same call boundaries (tools/flow_streams.py) and the CPU oracle; every call's segments are interleaved on the host by
tools/flow_mix.py (checked without a GPU in tests/test_flow_mix_cpu.py), with a pattern and a sprinkle of unrouted packets chosen per
call by a seeded generator.  offered, unrouted and left come from numpy models."""
import os
import sys

import numpy as np
import pytest

from ldpc_erasure_codes_amd import api, codes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_receiver import random_code, to_host  # noqa: E402
from test_gpu_flows import check, collect, same_runs, to_dev  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flow_mix as fm  # noqa: E402
import flow_streams as fs  # noqa: E402

EINVAL, ENOCODE = -1, -4
MIN_TILE, MAX_TILES = 1024, 1024


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


_CODES = {}


def get_code(ctx, which):
    """(handle, codes.Code), registered once with THIS module's context."""
    if which not in _CODES:
        if which == "rand":
            code = random_code()
            _CODES[which] = (ctx.register_code(code), code)
        else:
            _CODES[which] = (ctx.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which]), codes.load_builtin(which))
    return _CODES[which]


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


# ---------------------------------------------------------------------------------------------- 1. the partition alone
def lens_for(P, nflows, pattern, rng):
    """Packets per flow for a partition test: everything in one flow (single), a few long flows (runs), else a random split."""
    lens = np.zeros(nflows, dtype=np.int64)
    if pattern == "single":
        lens[rng.integers(0, nflows)] = P
    elif pattern == "runs":
        lens[:min(nflows, 3)] = np.bincount(rng.integers(0, min(nflows, 3), size=P), minlength=min(nflows, 3))
    elif pattern == "round_robin":
        lens[:] = P // nflows
        lens[:P - lens.sum()] += 1
    else:
        lens[:] = np.bincount(rng.integers(0, nflows, size=P), minlength=nflows)
    return lens


def ids_for(P, nflows, kind, unrouted, rng):
    if kind == "uniform":
        ids = rng.integers(0, nflows, size=P).astype(np.int32)
    elif kind == "last":
        ids = np.full(P, nflows - 1, dtype=np.int32)
    else:
        ids = fm.flow_ids(lens_for(P, nflows, kind, rng), kind, rng)
    return fm.sprinkle(ids, nflows, rng)[:max(P, 3)] if unrouted else ids   # (cut back to about P: the sizes are the point)


def partition_once(ctx, ids, nflows):
    """The library's partition of `ids` against numpy's stable sort; 64 guard words behind order."""
    L = ctx._L
    P = ids.size
    order = torch.full((P + 64,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    counts = np.full(nflows + 1, -7, dtype=np.int64)
    fo = dev_i32(ids)
    R = L.ldpc_amd_fec_flows_demux_dev(ctx._h, fo.data_ptr() if P else None, P, nflows, order.data_ptr(), counts.ctypes.data)
    want_order, want_counts, _ = fm.demux(ids, nflows)
    assert R == want_order.size, (P, nflows, R, L.ldpc_amd_last_error(ctx._h))
    got = order.cpu().numpy()
    assert np.array_equal(got[:R], want_order.astype(np.int32)), (P, nflows)
    assert (got[R:] == -0x5A5A5A5B).all(), (P, nflows, "order was written at or beyond the routed packets")
    assert np.array_equal(counts[:nflows], want_counts) and counts[nflows] == -7
    return ctx.fec_flows_demux_info()


@pytest.mark.parametrize("nflows", [1, 2, 64, 65, 4096])
def test_partition_is_numpys_stable_sort(ctx, nflows):
    rng = np.random.default_rng(100 + nflows)
    info = partition_once(ctx, np.zeros(1, dtype=np.int32), nflows)
    Lt = info["tile"]
    assert Lt == MIN_TILE and info["tiles"] == 1 and Lt % 64 == 0
    for P in (0, 1, 63, 64, 65, Lt - 1, Lt, Lt + 1, 3 * Lt + 17):
        for kind in fm.PATTERNS + ("uniform", "last"):
            for unrouted in (False, True):
                ids = ids_for(P, nflows, kind, unrouted, rng)
                info = partition_once(ctx, ids, nflows)
                assert info["tile"] == Lt and info["tiles"] == -(-ids.size // Lt), (P, kind, info)
    assert 0 < info["scratch_bytes"] <= 16 * (1 << 20) + 64 * 1024
    # the Python wrapper
    ids = ids_for(777, nflows, "uniform", True, rng)
    order, counts = ctx.fec_flows_demux(dev_i32(ids), nflows)
    want_order, want_counts, _ = fm.demux(ids, nflows)
    assert order.dtype == torch.int64 and np.array_equal(order.cpu().numpy(), want_order) and np.array_equal(counts, want_counts)


def test_partition_tile_grows_with_p(ctx):
    """Past MIN_TILE * MAX_TILES packets the tile grows instead of the table: ceil(P / 1024) rounded up to a multiple of 64."""
    nflows = 65
    rng = np.random.default_rng(9)
    P = MIN_TILE * MAX_TILES + 1
    ids = fm.sprinkle(rng.integers(0, nflows, size=P).astype(np.int32), nflows, rng, frac=0.01)
    ids[5000:9000] = 7                                    # a run longer than a tile, starting inside one
    info = partition_once(ctx, ids, nflows)
    tile = -(-(-(-ids.size // MAX_TILES)) // 64) * 64
    assert tile == 1088 and info["tile"] == tile != MIN_TILE and info["tiles"] == -(-ids.size // tile) <= MAX_TILES
    assert info["scratch_bytes"] <= 16 * (1 << 20) + 64 * 1024


# ---------------------------------------------------------------------------------------------- the receiver
MODES = ("decode_mixed", "decode_many", "push_mixed", "push_many")


def collect_mixed(ctx, h, code, S, sc, mode=lambda i: "decode_mixed", it=10, do_ml=1, seed=77, pattern=None, after=None, seen=None):
    """The stream set through ONE flows object over the reference run's call boundaries, call i through mode(i).  A mixed call gets
    the call's segments interleaved by a pattern (and with or without unrouted packets) drawn from a seeded generator; its offered,
    left and the object's unrouted count are checked here against numpy.  Returns what test_gpu_flows.collect returns."""
    nf = len(sc["flows"])
    rng = np.random.default_rng(seed)
    rx = ctx.fec_rx_flows(nf, code.n, code.k, S)
    res, unrouted, left_seen = [], 0, 0
    for i, call in enumerate(sc["calls"]):
        m = mode(i)
        segs = [sc["flows"][f][c["pos"]:c["pos"] + c["c"]] for f, c in enumerate(call["flows"])]
        pat = pattern or fm.PATTERNS[rng.integers(0, len(fm.PATTERNS))]
        sprinkle = bool(rng.integers(0, 2))
        fr = None
        if m.endswith("mixed"):
            pk_host, flow_of = fm.mix(segs, pat, seed + i, sprinkle)
            pk, fo = to_dev(pk_host), dev_i32(flow_of)
            if m == "decode_mixed":
                closes, blocks, fr, consumed, offered, left = rx.decode_mixed(h, pk, fo, call["mb"], max_sweeps=it, do_ml=do_ml, want_left=True)
            else:
                closes, blocks, sym, er, consumed, offered, left = rx.push_mixed(pk, fo, call["mb"], want_left=True)
            ctx.synchronize()
            unrouted += int(((flow_of < 0) | (flow_of >= nf)).sum())
            assert offered.dtype == np.int64 and np.array_equal(offered, [s.shape[0] for s in segs]), (i, offered)
            want_left = fm.left_model(flow_of, nf, consumed)
            assert np.array_equal(left.cpu().numpy(), want_left), (i, pat)
            left_seen += int(want_left.sum())
        else:
            pk_host, fb = fs.flow_begin_of(segs)
            pk = to_dev(pk_host)
            if m == "decode_many":
                closes, blocks, fr, consumed = rx.decode_many(h, pk, fb, call["mb"], max_sweeps=it, do_ml=do_ml)
            else:
                closes, blocks, sym, er, consumed = rx.push_many(pk, fb, call["mb"])
        if m.startswith("push"):
            fr = ctx.decode_frames(h, sym[:, :, 0].contiguous() if S == 1 else sym, er, max_sweeps=it, do_ml=do_ml) if len(blocks) else None
        ctx.synchronize()
        assert rx.unrouted == unrouted, (i, rx.unrouted, unrouted)
        r = dict(closes=closes, blocks=blocks, consumed=consumed, dropped=rx.dropped, frames=to_host(fr, S) if len(blocks) else None)
        if m.startswith("decode") and len(blocks):
            r["info"] = ctx.fec_receiver_info()
            if seen is not None and m == "decode_mixed":
                seen.update(plan=ctx.last_plan(), names=ctx.profile_kernel_names())
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
    return (res, flushes, dropped), dict(unrouted=unrouted, left=left_seen)


# ---------------------------------------------------------------------------------------------- 2. host receivers + oracle
def test_mixed_equals_host_receivers_and_oracle(ctx, oracle):
    h, code = get_code(ctx, "rand")
    oc = oracle.OracleCode(code)
    S = 16
    sc = fs.scenario("mixed", oc, code, S)
    got, seen = collect_mixed(ctx, h, code, S, sc)
    check(got, sc, oc, code, S, path="fused")          # closes, blocks, consumed, dropped, all six decoded arrays, the flushes
    assert seen["unrouted"] > 0 and seen["left"] > 0    # (offered, unrouted and left were compared call by call)
    assert (got[0][-1]["dropped"] > 0).any()


# ---------------------------------------------------------------------------------------------- 3. fused, tier 2 and the ML stage
def test_builtin_code_fused_with_tier2_and_ml_stage(ctx, oracle):
    h, code = get_code(ctx, 1)
    oc = oracle.OracleCode(code)
    S = 1024
    sc = fs.scenario("builtin", oc, code, S)
    seen = {}
    got, _ = collect_mixed(ctx, h, code, S, sc, it=1, seen=seen)   # one sweep leaves the 20 % flow's frames to tier 2 and the ML stage
    check(got, sc, oc, code, S, it=1, path="fused")
    assert all(r["info"]["path"] == "fused" for r in got[0] if "info" in r) and any("info" in r for r in got[0])
    plan, names = seen["plan"], seen["names"]
    assert names["apply"].startswith("ldpc_scatter_pktin_kernel<") and plan["two_tiers"] == 1
    lost = np.concatenate([fs.expected(c, code.n, S)["er"] for c in sc["calls"]]).sum(1)
    assert (lost > plan["tier1_cap"]).any() and names["apply_tier2"].startswith("ldpc_scatter_pktin_big_kernel<")


# ---------------------------------------------------------------------------------------------- 4. the composed paths
def test_composed_paths_give_the_same_bytes(oracle):
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        code = random_code()
        h = c.register_code(code)
        oc = oracle.OracleCode(code)
        sc1 = fs.scenario("mixed", oc, code, 1)
        check(collect_mixed(c, h, code, 1, sc1)[0], sc1, oc, code, 1, path="composed")       # S = 1
        sc = fs.scenario("mixed", oc, code, 16)
        c.configure("LDPC_AMD_RX_PKT", 0)
        try:
            check(collect_mixed(c, h, code, 16, sc)[0], sc, oc, code, 16, path="composed")   # the knob
        finally:
            c.configure("LDPC_AMD_RX_PKT", None)


# ---------------------------------------------------------------------------------------------- 5. free mixing
def test_mixed_and_segmented_calls_in_any_order(ctx, oracle):
    h, code = get_code(ctx, "rand")
    oc = oracle.OracleCode(code)
    S = 16
    sc = fs.scenario("mixed", oc, code, S)
    assert len(sc["calls"]) >= 2 * len(MODES)
    got, _ = collect_mixed(ctx, h, code, S, sc, mode=lambda i: MODES[i % len(MODES)], seed=5)
    ref = collect(ctx, h, code, S, sc)                  # a second object: segmented calls only
    same_runs(got, ref, "decode_mixed / decode_many / push_mixed / push_many in turn")
    got2, _ = collect_mixed(ctx, h, code, S, sc, mode=lambda i: MODES[(i + 2) % len(MODES)], seed=6)
    same_runs(got2, ref, "the same, push_mixed first")


# ---------------------------------------------------------------------------------------------- 6. many flows
def test_many_flows_strict_round_robin(ctx, oracle):
    h, code = get_code(ctx, "rand")
    oc = oracle.OracleCode(code)
    sc = fs.scenario("many", oc, code, 16)
    assert len(sc["flows"]) == 130 and len(sc["calls"]) == 1
    got, _ = collect_mixed(ctx, h, code, 16, sc, pattern="round_robin")
    check(got, sc, oc, code, 16, path="fused")


# ---------------------------------------------------------------------------------------------- 7. guard bands, refusals, P == 0
@pytest.mark.parametrize("knob", [None, 0])
def test_guard_bands_and_untouched_slots(ctx, oracle, knob):
    """A mixed call and the segmented call on the de-interleaved array write the same bytes into buffers that were filled with a
    pattern: every output, the slots at and beyond T, the guard bands around them -- and the guard bands around left."""
    h, code = get_code(ctx, "rand")
    n, k, S, nf, MB, G = code.n, code.k, 16, 3, 8, 4096
    flows = [f[0] for f in fs.equal_flows(oracle.OracleCode(code), code, S, nf, 5, 6000)]
    seg_host, fb = fs.flow_begin_of(flows)
    mix_host, flow_of = fm.mix(flows, "random", 11, unrouted=True)
    seg, pk, fo = to_dev(seg_host), to_dev(mix_host), dev_i32(flow_of)
    before = pk.clone()
    P = flow_of.size
    slots = nf * MB
    L = ctx._L
    sizes = dict(out=slots * n * S, sweeps=4 * slots, residual=4 * slots, status=4 * slots, erased_out=slots * n, residual_src=4 * slots,
                 sym=slots * n * S, er=slots * n, left=P)

    def run(mixed):
        bufs = {kk: torch.full((v + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda") for kk, v in sizes.items()}
        ptr = {kk: bufs[kk].data_ptr() + G for kk in bufs}
        blocks, closes = np.full(slots + 2, -7, dtype=np.int32), np.full(nf + 2, -7, dtype=np.int32)
        used, offered = np.full(nf + 2, -7, dtype=np.int64), np.full(nf + 2, -7, dtype=np.int64)
        dec = (ptr["out"], ptr["sweeps"], ptr["residual"], ptr["status"], ptr["erased_out"], ptr["residual_src"], blocks[1:].ctypes.data,
               closes[1:].ctypes.data, MB, used[1:].ctypes.data)
        with ctx.fec_rx_flows(nf, n, k, S) as rx:
            if mixed:
                T = L.ldpc_amd_fec_rx_flows_decode_mixed(rx._h, h, pk.data_ptr(), fo.data_ptr(), P, 10, 1, *dec, offered[1:].ctypes.data, ptr["left"])
            else:
                T = L.ldpc_amd_fec_rx_flows_decode_many(rx._h, h, seg.data_ptr(), fb.ctypes.data, 10, 1, *dec)
            ctx.synchronize()
            unrouted = rx.unrouted
        with ctx.fec_rx_flows(nf, n, k, S) as rx:
            if mixed:
                T2 = L.ldpc_amd_fec_rx_flows_push_mixed(rx._h, pk.data_ptr(), fo.data_ptr(), P, ptr["sym"], ptr["er"], None, None, MB, None, None, None)
            else:
                T2 = L.ldpc_amd_fec_rx_flows_push_many(rx._h, seg.data_ptr(), fb.ctypes.data, ptr["sym"], ptr["er"], None, None, MB, None)
            ctx.synchronize()
        assert T2 == T
        return T, {kk: b.cpu().numpy() for kk, b in bufs.items()}, blocks, closes, used, offered, unrouted

    ctx.configure("LDPC_AMD_RX_PKT", knob)
    try:
        T, a, blocks, closes, used, offered, unrouted = run(True)
        Ts, b, blocks_s, closes_s, used_s, _, _ = run(False)
    finally:
        ctx.configure("LDPC_AMD_RX_PKT", None)
    assert nf * 2 <= T < slots and T == Ts
    assert np.array_equal(blocks, blocks_s) and np.array_equal(closes, closes_s) and np.array_equal(used, used_s)
    assert np.array_equal(offered[1:1 + nf], np.diff(fb)) and offered[0] == -7 and (offered[1 + nf:] == -7).all()
    assert unrouted == P - fb[-1] > 0
    assert torch.equal(pk, before)                           # the packet array is only read
    for kk, v in sizes.items():
        assert (a[kk][:4096] == 0xA5).all() and (a[kk][4096 + v:] == 0xA5).all(), kk
        if kk != "left":
            assert np.array_equal(a[kk], b[kk]), kk          # (the segmented call's untouched slots are test_gpu_flows' subject)
            per = v // slots
            assert (a[kk][G + T * per:G + v] == 0xA5).all() and not (a[kk][G:G + T * per] == 0xA5).all(), kk
    assert not a["left"][G:G + P].any()                      # everything was consumed: MB was not reached


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
    pk_host, flow_of = fm.mix([pk[:40] for pk in sc["flows"]], "random", 3, unrouted=True)
    P = flow_of.size
    pk, fo = to_dev(pk_host), dev_i32(flow_of)
    left = torch.full((P,), 0xA5, dtype=torch.uint8, device="cuda")
    off2 = torch.zeros(4 * P + 8, dtype=torch.uint8, device="cuda")       # flow_of two bytes off 4-byte alignment
    off2[2:2 + 4 * P].copy_(fo.view(torch.uint8))
    assert (off2.data_ptr() + 2) % 4 == 2

    def refused(rc, want, text=None):
        assert rc == want, rc
        msg = L.ldpc_amd_last_error(ctx._h)
        assert msg and (text is None or text in msg), msg

    def after(i, rx):
        if i != 2:
            return
        state, unrouted = rx.dropped.copy(), rx.unrouted

        def dec(code_h=h, packets=pk.data_ptr(), fo_=fo.data_ptr(), P_=P, it=10, out_p=out.data_ptr(), mb=MB, left_p=left.data_ptr()):
            return L.ldpc_amd_fec_rx_flows_decode_mixed(rx._h, code_h, packets, fo_, P_, it, 1, out_p, i32[0].data_ptr(), i32[1].data_ptr(),
                                                        i32[2].data_ptr(), er.data_ptr(), i32[3].data_ptr(), None, None, mb, None, None, left_p)

        def push(packets=pk.data_ptr(), fo_=fo.data_ptr(), P_=P, sym_p=out.data_ptr(), mb=MB, left_p=left.data_ptr()):
            return L.ldpc_amd_fec_rx_flows_push_mixed(rx._h, packets, fo_, P_, sym_p, er.data_ptr(), None, None, mb, None, None, left_p)

        for call in (dec, push):
            refused(call(fo_=None), EINVAL, b"flow_of")
            refused(call(fo_=flow_of.ctypes.data), EINVAL, b"flow_of must be a device pointer")
            refused(call(fo_=off2.data_ptr() + 2), EINVAL, b"4-byte aligned")
            refused(call(P_=-1), EINVAL, b"2^31")
            refused(call(P_=1 << 31), EINVAL, b"2^31")
            refused(call(mb=0), EINVAL, b"max_blocks_per_flow")
            refused(call(mb=(1 << 31) // (nf * n) + 1), EINVAL, b"2^31 - 2")
            refused(call(packets=pk_host.ctypes.data), EINVAL, b"device pointer")
            refused(call(left_p=out_host.ctypes.data), EINVAL, b"left must be a device pointer")
        refused(push(sym_p=out_host.ctypes.data), EINVAL, b"device pointers")
        refused(dec(out_p=out_host.ctypes.data), EINVAL, b"device pointers")
        refused(dec(code_h=hb), EINVAL, b"(2040,1530)")
        refused(dec(code_h=999), ENOCODE, b"unknown code handle")
        refused(dec(it=0), EINVAL, b"max_sweeps must be >= 1")
        # P == 0: returns 0, zeroes closes / consumed / offered, nothing else is touched (not even looked at)
        cl, us, of = np.full(nf, -7, dtype=np.int32), np.full(nf, -7, dtype=np.int64), np.full(nf, -7, dtype=np.int64)
        assert L.ldpc_amd_fec_rx_flows_decode_mixed(rx._h, h, None, None, 0, 10, 1, None, None, None, None, None, None, None, cl.ctypes.data, MB,
                                                    us.ctypes.data, of.ctypes.data, None) == 0
        assert (cl == 0).all() and (us == 0).all() and (of == 0).all()
        of[:] = -7
        assert L.ldpc_amd_fec_rx_flows_push_mixed(rx._h, None, None, 0, out.data_ptr(), er.data_ptr(), None, None, MB, None, of.ctypes.data,
                                                  left.data_ptr()) == 0
        assert (of == 0).all()
        ctx.synchronize()
        assert bool((out == 0xA5).all()) and bool((er == 0xA5).all()) and bool((left == 0xA5).all())
        assert np.array_equal(rx.dropped, state) and rx.unrouted == unrouted

    # the partition's own refusals
    order = torch.zeros(P, dtype=torch.int32, device="cuda")
    for bad_nf in (0, -1, 4097):
        refused(L.ldpc_amd_fec_flows_demux_dev(ctx._h, fo.data_ptr(), P, bad_nf, order.data_ptr(), None), EINVAL, b"nflows")
    refused(L.ldpc_amd_fec_flows_demux_dev(ctx._h, fo.data_ptr(), 1 << 31, nf, order.data_ptr(), None), EINVAL, b"2^31")
    refused(L.ldpc_amd_fec_flows_demux_dev(ctx._h, flow_of.ctypes.data, P, nf, order.data_ptr(), None), EINVAL, b"device pointers")
    refused(L.ldpc_amd_fec_flows_demux_dev(ctx._h, off2.data_ptr() + 2, P, nf, order.data_ptr(), None), EINVAL, b"4-byte aligned")
    refused(L.ldpc_amd_fec_flows_demux_info(ctx._h, None), EINVAL)
    # every refusal in the middle of the stream: the calls before and behind it return the reference's values
    got, _ = collect_mixed(ctx, h, code, S, sc, after=after)
    check(got, sc, oc, code, S, path="fused")
