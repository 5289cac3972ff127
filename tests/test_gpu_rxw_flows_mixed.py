"""GPU tests of the mixed calls of the windowed multi-flow receiver (include/ldpc_erasure_amd_rx_window_flows_mixed.h): packets of
many flows in ONE array in arrival order, a flow number per packet.

The expected values never come from the code under test: one api.FecRxWindowHost per flow (tests/rxw_flows_cases.py: HostFlows) over
the same calls, tools/flow_mix.py for the interleaving, its inverse and the `left` model, and the CPU oracle for decoded frames.
tests/test_rxw_flows_mixed_cases_cpu.py shows that the interleaved schedules hold the cases they are meant to."""
import ctypes as C

import numpy as np
import pytest

import rxw_cases as rc
import rxw_flows_cases as fc
import rxw_flows_mixed_cases as mc
from ldpc_erasure_codes_amd import api

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_rx_window import oracle_frames  # noqa: E402
from test_gpu_rxw_flows import (NAMES, coded_stream, dev, dev_at, get_code, raw_flush, raw_push, same_flows, same_flush, same_frames,  # noqa: E402
                                same_push, single_flow_path, to_host)

fm = mc.fm
wm = rc.wm
N, K = rc.N, rc.K
EINVAL, ENOCODE = -1, -4
GUARD = 0xA5
BAND = 64   # guard bytes on either side of `left`


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def raw_push_mixed(rx, d_pk, d_fo, mb):
    """ldpc_amd_fec_rxw_flows_push_mixed into the middle of guarded buffers: ((closes, blocks [T], sym [T], er [T], consumed), offered,
    left [P]); asserts that the bands around the outputs, the slots at or beyond T and the bands around left are untouched."""
    n, S, nf = rx.n, rx.S, rx.nflows
    P = d_pk.shape[0]
    slots = nf * mb
    sym = torch.full((slots + 2, n, S), GUARD, dtype=torch.uint8, device="cuda")
    er = torch.full((slots + 2, n), GUARD, dtype=torch.uint8, device="cuda")
    left = torch.full((P + 2 * BAND,), GUARD, dtype=torch.uint8, device="cuda")
    blocks = np.full(slots + 1, -7, dtype=np.int32)
    closes = np.full(nf + 1, -7, dtype=np.int32)
    consumed, offered = np.full(nf + 1, -7, dtype=np.int64), np.full(nf + 1, -7, dtype=np.int64)
    T = rx._ctx._check(rx._L.ldpc_amd_fec_rxw_flows_push_mixed(
        rx._h, d_pk.data_ptr() if P else None, d_fo.data_ptr() if P else None, P, sym[1].data_ptr(), er[1].data_ptr(), blocks.ctypes.data,
        closes.ctypes.data, mb, consumed.ctypes.data, offered.ctypes.data, left.data_ptr() + BAND), "fec_rxw_flows_push_mixed")
    rx._ctx.synchronize()
    for t in (sym, er):
        assert bool((t[0] == GUARD).all()) and bool((t[1 + T:] == GUARD).all()), "guard bands and unused slots are untouched"
    assert (blocks[T:] == -7).all() and closes[nf] == -7 and consumed[nf] == -7 and offered[nf] == -7
    lf = left.cpu().numpy()
    assert (lf[:BAND] == GUARD).all() and (lf[BAND + P:] == GUARD).all(), "the bands around left are untouched"
    return (closes[:nf], blocks[:T], sym[1:1 + T].cpu().numpy(), er[1:1 + T].cpu().numpy(), consumed[:nf]), offered[:nf], lf[BAND:BAND + P]


def same_mixed(rx, got, call, flow_of, tag):
    """One mixed call against the host objects' call and the numpy models of offered and left."""
    res, offered, left = got
    same_push(res, call, tag)
    assert np.array_equal(offered, [p.shape[0] for p in call.pieces]), tag
    assert np.array_equal(left, fm.left_model(flow_of, rx.nflows, call.consumed)), tag


# ------------------------------------------------------------------------------------------------------ 1. lockstep
@pytest.mark.parametrize("W,A", fc.LOCKSTEP_WA)
@pytest.mark.parametrize("nflows", fc.LOCKSTEP_NFLOWS)
def test_lockstep_with_host_objects(ctx, nflows, W, A):
    """The lockstep schedule of the segmented test with every call interleaved (pattern and unrouted packets by the call's number),
    every third call segmented: after every call closes, blocks, bytes, flags, consumed, offered, left, the unrouted count and per
    flow totals, state and dropped; then the flush."""
    streams = fc.lockstep_streams(nflows, A)
    seed = fc.lockstep_seed(nflows, W, A)
    unrouted = left_ones = mixed_calls = 0
    with ctx.fec_rx_window_flows(nflows, N, K, rc.S, W, A) as rx, fc.HostFlows(nflows, W, A) as hx:
        for i, call in enumerate(fc.lockstep_calls(hx, streams, seed)):
            tag = (nflows, W, A, i, call.mb)
            if i % 3 == 2:
                pk, fb = fc.concat(call.pieces)
                same_push(raw_push(rx, dev(pk), fb, call.mb), call, tag)
            else:
                pk, flow_of = mc.mixed_call(call, i, seed)
                got = raw_push_mixed(rx, dev(pk), dev_i32(flow_of), call.mb)
                same_mixed(rx, got, call, flow_of, tag)
                unrouted += mc.unrouted_in(flow_of, nflows)
                left_ones += int(got[2].sum())
                mixed_calls += 1
            assert rx.unrouted == unrouted, tag
            same_flows(rx, hx, tag)
        assert rx.pending().blocks == sum(hx.pending())
        same_flush(rx, hx, None, "flush")
        same_flows(rx, hx, "flush")
        assert same_flush(rx, hx, None, "second flush") == 0
        assert rx.unrouted == unrouted
    assert mixed_calls >= 6 and unrouted > 0 and left_ones > 0


# ------------------------------------------------------------------------------------------------------ 2. data paths
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("S", [1, 20, 16, 1024])
def test_data_paths(ctx, S, odd):
    """The 16-byte path and the byte path of the gather and the staging update, and both forms of the header read, behind the
    permutation; duplicates of a flow with a flipped payload, other flows' packets between them: the last copy in arrival order wins;
    blocks carried in the staging planes from one call to a later one."""
    nflows, W, A, mb = 3, 4, 10, 3
    streams = [rc.random_stream(rc.RANDOM_SEEDS[2 + f], S=S) for f in range(nflows)]
    hdr = [wm.headers(pk) for pk in streams]
    for pk, (blk, sym) in zip(streams, hdr):
        assert np.unique(np.stack([blk, sym]), axis=1).shape[1] < pk.shape[0], "the stream holds duplicates (their payload is flipped)"
    carried = 0
    with ctx.fec_rx_window_flows(nflows, N, K, S, W, A) as rx, fc.HostFlows(nflows, W, A, S_=S) as hx:
        for i, call in enumerate(fc.lockstep_calls(hx, streams, 5, sizes=(300, 17, 1111, 64, 2000), mbs=(mb,))):
            pk, flow_of = fm.mix(call.pieces, ("random", "round_robin")[i & 1], 40 + i, unrouted=bool(i & 2))
            same_mixed(rx, raw_push_mixed(rx, dev_at(pk, odd), dev_i32(flow_of), mb), call, flow_of, (S, odd, i))
            slot = 0
            for f, (a, _) in enumerate(call.spans):
                blk, sym = hdr[f][0][a:a + call.consumed[f]], hdr[f][1][a:a + call.consumed[f]]
                for j in range(slot, slot + call.closes[f]):
                    here = np.unique(sym[(blk == call.blocks[j]) & (sym < N)]).size
                    carried += int(N - call.er[j].sum() > here)
                slot += call.closes[f]
        assert carried >= 3, "closed blocks that hold rows an earlier call received"
        same_flows(rx, hx, "end")
        assert same_flush(rx, hx, None, "flush") >= nflows


# ------------------------------------------------------------------------------------------------------ 3. decode
def decode_three_ways(ctx, oc, h, code, S, streams, W, A, mb=3, sizes=(700, 2500, 10 ** 9)):
    """Three objects over the same calls: decode_mixed; push_mixed + Context.decode_frames; segmented decode_many on the array
    de-interleaved on the host.  Everything the calls return must be equal, and (oc) equal to the oracle on the gathered symbols.
    Returns (blocks closed, the forms decode_mixed reported)."""
    nf = len(streams)
    pos, paths, closed, i, left_ones = [0] * nf, set(), 0, 0, 0
    mk = lambda: ctx.fec_rx_window_flows(nf, code.n, code.k, S, W, A)   # noqa: E731
    with mk() as rd, mk() as rp, mk() as rs:
        while any(pos[f] < streams[f].shape[0] for f in range(nf)):
            pieces = [streams[f][pos[f]:pos[f] + sizes[(i + f) % len(sizes)]] for f in range(nf)]
            pk, flow_of = fm.mix(pieces, fm.PATTERNS[i % len(fm.PATTERNS)], 900 + i, unrouted=bool(i & 1), run=300)
            d_pk, d_fo = dev(pk), dev_i32(flow_of)
            c1, b1, fr, u1, o1, l1 = rd.decode_mixed(h, d_pk, d_fo, mb, want_left=True)
            info = ctx.fec_rx_window_flows_info()
            c0, b0, sym, er, u0, o0, l0 = rp.push_mixed(d_pk, d_fo, mb, want_left=True)
            seg, fb = mc.deinterleave(pk, flow_of, nf)
            d_seg = dev(seg)
            c2, b2, fr2, u2 = rs.decode_many(h, d_seg, fb, mb)
            for c, b, u in ((c0, b0, u0), (c2, b2, u2)):
                assert np.array_equal(c, c1) and np.array_equal(b, b1) and np.array_equal(u, u1), i
            assert u1.sum() > 0 and np.array_equal(o1, np.diff(fb)) and np.array_equal(o0, o1), i
            want_left = fm.left_model(flow_of, nf, u1)
            assert np.array_equal(l1.cpu().numpy(), want_left) and torch.equal(l0, l1), i
            left_ones += int(want_left.sum())
            assert info["blocks"] == len(b1)
            paths.add(info["path"])
            if len(b1):
                got = to_host(fr, S)
                same_frames(got, to_host(ctx.decode_frames(h, sym, er), S), ("push_mixed + decode_frames", i))
                same_frames(got, to_host(fr2, S), ("decode_many on the de-interleaved array", i))
                assert info["launches"] >= 1
                if oc is not None:
                    for name, a, w in zip(NAMES[:4], got[:4], oracle_frames(oc, sym.cpu().numpy(), er.cpu().numpy())):
                        assert np.array_equal(a, w), ("oracle", i, name)
            for f in range(nf):
                pos[f] += int(u1[f])
            closed += len(b1)
            i += 1
        assert rd.unrouted == rp.unrouted > 0 and rs.unrouted == 0 and left_ones > 0
        for f in range(nf):
            assert rd.stats(f) == rp.stats(f) and rd.state(f) == rp.state(f)
        c1, b1, fr = rd.decode_flush_many(h)
        c2, b2, fr2 = rs.decode_flush_many(h)
        assert np.array_equal(c1, c2) and np.array_equal(b1, b2) and len(b1) >= 1
        same_frames(to_host(fr, S), to_host(fr2, S), "decode_flush_many")
        for f in range(nf):
            assert rd.stats(f) == rs.stats(f) and rd.state(f) == rs.state(f)
    return closed + len(b1), paths


@pytest.mark.parametrize("which,F", [("rand", 12), (1, 5)])
def test_decode_mixed_three_ways_and_the_oracle(ctx, oracle, which, F):
    """decode_mixed == push_mixed + decode_frames == decode_many on the de-interleaved array == the oracle on the gathered symbols,
    fused and composed (the rx_pkt knob); the info call reports the form the segmented call takes."""
    S, W, A, nf = 16, 4, 10, 3
    h, code = get_code(ctx, which)
    oc = oracle.OracleCode(code)
    streams = [coded_stream(ctx, h, code, S, F, seed=600 + 10 * f + F, block0=(250 + 40 * f) & 0xFF, loss=0.10, window=code.n // 2, dup=0.02)
               for f in range(nf)]
    closed, paths = decode_three_ways(ctx, oc, h, code, S, streams, W, A)
    assert closed >= nf * (F - 1)
    want = single_flow_path(ctx, h, code, S, streams[0], W, A)
    assert paths == {want}
    if which == 1:
        assert want == "fused"
    ctx.configure("LDPC_AMD_RX_PKT", 0)
    try:
        closed0, paths0 = decode_three_ways(ctx, None, h, code, S, streams, W, A)
    finally:
        ctx.configure("LDPC_AMD_RX_PKT", None)
    assert closed0 == closed and paths0 == {"composed"}


# ------------------------------------------------------------------------------------------------------ 4. edges of the partition
def long_streams(nflows, blocks=60):
    return [rc.through_link(rc.packets_of(*rc.sent(blocks, lambda b: 0.93, 20 + f, block0=(90 * f) & 0xFF), seed=f), 30 + f, window=150, dup=0.02)
            for f in range(nflows)]


@pytest.mark.parametrize("pattern", ["round_robin", "runs", "reverse"])
def test_partition_edges_inside_the_receiver(ctx, pattern):
    """Single calls of P around the group of 64 lanes and the tile of 1024 packets, then a large call, a small one and a larger one
    (the index scratch grows again), on one object."""
    nflows, W, A, mb = 3, 4, 10, 64
    streams = long_streams(nflows)
    pos = [0] * nflows
    big = 3 * 1024 + 17
    with ctx.fec_rx_window_flows(nflows, N, K, rc.S, W, A) as rx, fc.HostFlows(nflows, W, A) as hx:
        for i, P in enumerate((1, 63, 64, 65, 1023, 1024, 1025, big, 5, 2 * big)):
            lens = [P // nflows + (1 if f < P % nflows else 0) for f in range(nflows)]
            pieces = [streams[f][pos[f]:pos[f] + lens[f]] for f in range(nflows)]
            assert [p.shape[0] for p in pieces] == lens, "the streams are long enough"
            call = fc.Call(mb, None, pieces, *hx.push_many(pieces, mb))
            pk, flow_of = fm.mix(pieces, pattern, 70 + i, unrouted=False, run=fm.RUN if P > 2 * fm.RUN else mc.SHORT_RUN)
            assert flow_of.size == P
            same_mixed(rx, raw_push_mixed(rx, dev(pk), dev_i32(flow_of), mb), call, flow_of, (pattern, P))
            same_flows(rx, hx, (pattern, P))
            for f in range(nflows):
                pos[f] += int(call.consumed[f])
        assert rx.unrouted == 0
        assert same_flush(rx, hx, None, "flush") >= nflows


def test_a_call_of_unrouted_packets_only(ctx):
    """Returns 0, every flow unchanged, left all zero, unrouted advanced by P."""
    nflows, W, A, mb = 3, 4, 10, 4
    streams = fc.lockstep_streams(nflows, A)
    first = [pk[:700] for pk in streams]
    rest = [pk[700:1900] for pk in streams]
    with ctx.fec_rx_window_flows(nflows, N, K, rc.S, W, A) as rx, fc.HostFlows(nflows, W, A) as hx:
        pk, flow_of = fm.mix(first, "random", 1)
        call = fc.Call(mb, None, first, *hx.push_many(first, mb))
        same_mixed(rx, raw_push_mixed(rx, dev(pk), dev_i32(flow_of), mb), call, flow_of, "first")
        before = [(rx.state(f), rx.stats(f)) for f in range(nflows)]
        P = 1300
        ids = np.array([-1, nflows, 2 ** 31 - 1, -2 ** 31, 4096], dtype=np.int64)[np.random.default_rng(2).integers(0, 5, size=P)].astype(np.int32)
        noise = np.random.default_rng(3).integers(0, 256, size=(P, 8 + rc.S), dtype=np.uint8)
        (closes, blocks, sym, er, consumed), offered, left = raw_push_mixed(rx, dev(noise), dev_i32(ids), mb)
        assert len(blocks) == 0 and not closes.any() and not consumed.any() and not offered.any() and not left.any()
        assert rx.unrouted == P and [(rx.state(f), rx.stats(f)) for f in range(nflows)] == before
        same_flows(rx, hx, "after the unrouted call")
        pk, flow_of = fm.mix(rest, "runs", 4, unrouted=True, run=mc.SHORT_RUN)
        call = fc.Call(mb, None, rest, *hx.push_many(rest, mb))
        same_mixed(rx, raw_push_mixed(rx, dev(pk), dev_i32(flow_of), mb), call, flow_of, "the next call")
        same_flows(rx, hx, "the next call")
        assert rx.unrouted == P + mc.unrouted_in(flow_of, nflows)


def test_4096_flows_four_of_them_busy(ctx):
    """nflows = 4096, W = 2: packets only in flows 0, 63, 64 and 4095, the first and last lane of the first chunk of flow numbers,
    the first of the second, and the last flow of all."""
    nflows, W, A, mb = 4096, 2, 0, 2
    busy = (0, 63, 64, 4095)
    src = long_streams(len(busy), blocks=12)
    none = np.zeros((0, 8 + rc.S), np.uint8)
    with ctx.fec_rx_window_flows(nflows, N, K, rc.S, W, A) as rx, fc.HostFlows(nflows, W, A) as hx:
        pos = [0] * len(busy)
        for i, take in enumerate((900, 1300)):
            pieces = [none] * nflows
            for j, f in enumerate(busy):
                pieces[f] = src[j][pos[j]:pos[j] + take]
            call = fc.Call(mb, None, pieces, *hx.push_many(pieces, mb))
            pk, flow_of = fm.mix(pieces, ("random", "round_robin")[i], 8 + i, unrouted=True)
            same_mixed(rx, raw_push_mixed(rx, dev(pk), dev_i32(flow_of), mb), call, flow_of, i)
            for j, f in enumerate(busy):
                pos[j] += int(call.consumed[f])
                assert (rx.state(f), rx.stats(f)) == (hx.state(f), hx.stats(f)), (i, f)
            assert call.closes.sum() >= len(busy) and rx.pending().blocks == sum(hx.pending())
        for f in (1, 62, 65, 4094):
            assert rx.state(f)["base"] == -1
        assert same_flush(rx, hx, list(busy), "flush") >= len(busy)


# ------------------------------------------------------------------------------------------------------ 5. the closed loop
def test_closed_loop_sender_link_receiver(ctx):
    """FecTxFlows (round robin) -> FecLink with flow_of -> decode_mixed, the `left` packets submitted again until none remain, then
    decode_flush_many: the output is that of a second object fed the same arrivals de-interleaved on the host through decode_many,
    and every frame whose status reports complete carries the sent source rows."""
    S, nf, F, W, A, mb = 16, 5, 6, 8, 10, 2
    h, code = get_code(ctx, "rand")
    block0 = [0, 250, 100, 255, 7]
    source = torch.randint(0, 256, (nf * F, code.k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(21))
    pk, flow_of, _ = ctx.fec_tx_flows(h, S, nf, block0=block0).send(source, np.arange(nf + 1) * F, api.TX_ROUND_ROBIN)
    P = pk.shape[0]
    lost = ctx.synth_erasures_uniform(31, 0, P, 1, 0.10, torch.empty(P, dtype=torch.uint8, device="cuda"))
    arrived, fo, _, _ = ctx.fec_link(32, window=300, dup=0.02, bad_sym=0.01).send(pk, lost, flow_of)
    src_host = source.cpu().numpy()
    pk_host, fo_host = arrived.cpu().numpy(), fo.cpu().numpy()
    assert not np.array_equal(np.sort(fo_host, kind="stable"), fo_host), "the arrivals are interleaved"
    segs = [pk_host[fo_host == f] for f in range(nf)]
    complete = rounds = left_ones = 0

    def sent_rows(got, blocks, closes, tag):
        nonlocal complete
        at = np.concatenate([[0], np.cumsum(closes)])
        assert len(closes) == nf
        for f in range(nf):
            for j in range(at[f], at[f + 1]):
                if got[3][j] <= 1:   # MP_DONE / ML_SOLVED
                    idx = (int(blocks[j]) - block0[f]) & 0xFF
                    assert idx < F and np.array_equal(got[0][j, :code.k], src_host[f * F + idx]), (tag, f, j)
                    complete += 1

    with ctx.fec_rx_window_flows(nf, code.n, code.k, S, W, A) as rx, ctx.fec_rx_window_flows(nf, code.n, code.k, S, W, A) as ref:
        d_pk, d_fo = arrived.contiguous(), fo.contiguous()
        while d_pk.shape[0] > 0:
            rounds += 1
            assert rounds <= 4 * F, "every round closes blocks or consumes every packet"
            closes, blocks, fr, consumed, offered, left = rx.decode_mixed(h, d_pk, d_fo, mb, want_left=True)
            seg, fb = fc.concat(segs, S)
            c2, b2, fr2, u2 = ref.decode_many(h, dev(seg), fb, mb)
            assert np.array_equal(closes, c2) and np.array_equal(blocks, b2) and np.array_equal(consumed, u2), rounds
            assert np.array_equal(offered, np.diff(fb)), rounds
            got = to_host(fr, S)
            same_frames(got, to_host(fr2, S), ("round", rounds))
            sent_rows(got, blocks, closes, ("round", rounds))
            segs = [s[int(u):] for s, u in zip(segs, u2)]
            keep = left.bool()
            left_ones += int(keep.sum())
            assert int(keep.sum()) == sum(s.shape[0] for s in segs)
            d_pk, d_fo = d_pk[keep].contiguous(), d_fo[keep].contiguous()
        assert rounds >= 2 and left_ones > 0
        closes, blocks, fr = rx.decode_flush_many(h)
        c2, b2, fr2 = ref.decode_flush_many(h)
        assert np.array_equal(closes, c2) and np.array_equal(blocks, b2)
        got = to_host(fr, S)
        same_frames(got, to_host(fr2, S), "flush")
        sent_rows(got, blocks, closes, "flush")
        for f in range(nf):
            assert rx.stats(f) == ref.stats(f) and rx.state(f) == ref.state(f)
        assert rx.unrouted == 0 and rx.pending().blocks == 0
    assert complete >= 1


# ------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_are_atomic(ctx):
    L = ctx._L
    code_h, _ = get_code(ctx, "rand")   # (300, 200): not the object's (n, k)
    nf, W, A, mb = 3, 4, 10, 4
    streams = fc.lockstep_streams(nf, A)
    first = [pk[:1000] for pk in streams]
    rest = [pk[1000:] for pk in streams]
    with ctx.fec_rx_window_flows(nf, N, K, rc.S, W, A) as rx, fc.HostFlows(nf, W, A) as hx:
        pk, flow_of = fm.mix(first, "random", 12, unrouted=True)
        call = fc.Call(64, None, first, *hx.push_many(first, 64))
        same_mixed(rx, raw_push_mixed(rx, dev(pk), dev_i32(flow_of), 64), call, flow_of, "first")

        def snapshot():
            p = rx.pending()
            return [(rx.state(f), rx.stats(f)) for f in range(nf)], p.base.tolist(), p.cnt.tolist(), p.blocks, rx.unrouted

        before = snapshot()
        assert before[3] > 0 and before[4] > 0
        pk, flow_of = fm.mix(rest, "round_robin", 13, unrouted=True)
        P = flow_of.size
        d_pk, d_fo = dev(pk), dev_i32(flow_of)
        slots = nf * mb
        sym = torch.full((slots, N, rc.S), GUARD, dtype=torch.uint8, device="cuda")
        er = torch.full((slots, N), GUARD, dtype=torch.uint8, device="cuda")
        out = torch.full((slots, 300, rc.S), GUARD, dtype=torch.uint8, device="cuda")
        left = torch.full((P,), GUARD, dtype=torch.uint8, device="cuda")
        host = np.zeros((slots, 300, rc.S), dtype=np.uint8)
        off2 = torch.zeros(4 * P + 8, dtype=torch.uint8, device="cuda")       # flow_of two bytes off 4-byte alignment
        off2[2:2 + 4 * P].copy_(d_fo.view(torch.uint8))
        assert (off2.data_ptr() + 2) % 4 == 2
        closes, used, offered = np.zeros(nf, np.int32), np.zeros(nf, np.int64), np.zeros(nf, np.int64)

        def push(packets=d_pk.data_ptr(), fo_=d_fo.data_ptr(), P_=P, s=sym.data_ptr(), m=mb, left_p=left.data_ptr()):
            return L.ldpc_amd_fec_rxw_flows_push_mixed(rx._h, packets, fo_, P_, s, er.data_ptr(), None, closes.ctypes.data, m, used.ctypes.data,
                                                       offered.ctypes.data, left_p)

        def decode(code=code_h, fo_=d_fo.data_ptr(), P_=P, m=mb, o=out.data_ptr(), left_p=left.data_ptr()):
            return L.ldpc_amd_fec_rxw_flows_decode_mixed(rx._h, code, d_pk.data_ptr(), fo_, P_, 10, 1, o, None, None, None, None, None, None,
                                                         closes.ctypes.data, m, used.ctypes.data, offered.ctypes.data, left_p)

        refused = [(lambda: push(fo_=None), EINVAL, b"flow_of"), (lambda: push(fo_=flow_of.ctypes.data), EINVAL, b"flow_of must be a device pointer"),
                   (lambda: push(fo_=off2.data_ptr() + 2), EINVAL, b"4-byte aligned"),
                   (lambda: push(left_p=host.ctypes.data), EINVAL, b"left must be a device pointer"),
                   (lambda: push(P_=-1), EINVAL, b"2^31"), (lambda: push(P_=1 << 31), EINVAL, b"2^31"),
                   (lambda: push(m=0), EINVAL, b"max_blocks_per_flow"),
                   (lambda: push(packets=pk.ctypes.data), EINVAL, b"device pointers"), (lambda: push(s=host.ctypes.data), EINVAL, b"device pointers"),
                   (lambda: decode(), EINVAL, b"the code is (300,200)"), (lambda: decode(code=999), ENOCODE, b"unknown code handle"),
                   (lambda: decode(fo_=None), EINVAL, b"the code is"), (lambda: decode(P_=-1), EINVAL, b"2^31"),
                   (lambda: decode(P_=1 << 31), EINVAL, b"2^31"), (lambda: decode(m=0), EINVAL, b"max_blocks_per_flow")]
        for i, (call_, want, text) in enumerate(refused):
            assert call_() == want and text in L.ldpc_amd_last_error(ctx._h), (i, text, L.ldpc_amd_last_error(ctx._h))
            assert snapshot() == before, (i, text)
        # the mixed calls' own checks in decode_mixed, on an object of the code's (n, k)
        with ctx.fec_rx_window_flows(nf, 300, 200, rc.S, W, A) as r2:
            noise = torch.zeros((P, 8 + rc.S), dtype=torch.uint8, device="cuda")
            out2 = torch.full((slots, 300, rc.S), GUARD, dtype=torch.uint8, device="cuda")

            def dec2(fo_=d_fo.data_ptr(), left_p=left.data_ptr()):
                return L.ldpc_amd_fec_rxw_flows_decode_mixed(r2._h, code_h, noise.data_ptr(), fo_, P, 10, 1, out2.data_ptr(), None, None, None, None,
                                                             None, None, None, mb, None, None, left_p)

            for call_, text in [(lambda: dec2(fo_=None), b"flow_of"), (lambda: dec2(fo_=flow_of.ctypes.data), b"flow_of must be a device pointer"),
                                (lambda: dec2(fo_=off2.data_ptr() + 2), b"4-byte aligned"),
                                (lambda: dec2(left_p=host.ctypes.data), b"left must be a device pointer")]:
                assert call_() == EINVAL and text in L.ldpc_amd_last_error(ctx._h), text
                assert r2.unrouted == 0 and r2.pending().blocks == 0 and all(r2.state(f)["base"] == -1 for f in range(nf))
            ctx.synchronize()
            assert bool((out2 == GUARD).all())
        # P == 0: returns 0, zeroes closes / consumed / offered, nothing else is touched (not even looked at)
        closes[:], used[:], offered[:] = -7, -7, -7
        assert L.ldpc_amd_fec_rxw_flows_decode_mixed(rx._h, code_h, None, None, 0, 10, 1, None, None, None, None, None, None, None,
                                                     closes.ctypes.data, mb, used.ctypes.data, offered.ctypes.data, None) == 0
        assert not closes.any() and not used.any() and not offered.any()
        closes[:], used[:], offered[:] = -7, -7, -7
        assert push(packets=None, fo_=None, P_=0) == 0
        assert not closes.any() and not used.any() and not offered.any()
        ctx.synchronize()
        assert bool((sym == GUARD).all()) and bool((er == GUARD).all()) and bool((out == GUARD).all()) and bool((left == GUARD).all())
        assert snapshot() == before
        call = fc.Call(mb, None, rest, *hx.push_many(rest, mb))
        same_mixed(rx, raw_push_mixed(rx, d_pk, d_fo, mb), call, flow_of, "the next good call")
        same_flows(rx, hx, "the next good call")
        assert rx.unrouted == before[4] + mc.unrouted_in(flow_of, nf)
