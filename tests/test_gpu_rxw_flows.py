"""GPU tests of the windowed multi-flow receiver (include/ldpc_erasure_amd_rx_window_flows.h, csrc/rx_window_flows_dev.hip).  The
reference of every comparison is one api.FecRxWindowHost per flow (tests/rxw_flows_cases.py: HostFlows), byte for byte; decoded frames
are compared with Context.decode_frames on the blocks push_many / flush_many hand out.  tests/test_rxw_flows_cases_cpu.py shows that the
streams and schedules used here hold the cases they are meant to."""
import ctypes as C

import numpy as np
import pytest

import rxw_cases as rc
import rxw_flows_cases as fc
from code_helpers import random_code
from ldpc_erasure_codes_amd import api, codes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

wm = rc.wm
N, K = rc.N, rc.K
EINVAL = -1
GUARD = 0xA5
NAMES = ("out", "sweeps", "residual", "status", "erased_out", "residual_src")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_at(pk, odd):
    """The packet array on the device at an even (16-byte aligned) or an odd address."""
    P, plen = pk.shape
    buf = torch.zeros(P * plen + 32, dtype=torch.uint8, device="cuda")
    off = 1 if odd else 0
    d = buf[off:off + P * plen].view(P, plen)
    d.copy_(dev(pk))
    assert P == 0 or d.data_ptr() % 2 == off
    return d


def raw_push(rx, d_pk, fb, mb):
    """ldpc_amd_fec_rxw_flows_push_many into the middle of guarded buffers: (closes, blocks [T], sym [T], er [T], consumed); asserts
    that the bands around the output and the slots at or beyond T are untouched."""
    n, S, nf = rx.n, rx.S, rx.nflows
    slots = nf * mb
    sym = torch.full((slots + 2, n, S), GUARD, dtype=torch.uint8, device="cuda")
    er = torch.full((slots + 2, n), GUARD, dtype=torch.uint8, device="cuda")
    blocks = np.full(slots + 1, -7, dtype=np.int32)
    closes, consumed = np.full(nf + 1, -7, dtype=np.int32), np.full(nf + 1, -7, dtype=np.int64)
    fb = np.ascontiguousarray(fb, dtype=np.int64)
    T = rx._ctx._check(rx._L.ldpc_amd_fec_rxw_flows_push_many(rx._h, d_pk.data_ptr() if d_pk.shape[0] else None, fb.ctypes.data, sym[1].data_ptr(),
                                                              er[1].data_ptr(), blocks.ctypes.data, closes.ctypes.data, mb, consumed.ctypes.data),
                       "fec_rxw_flows_push_many")
    rx._ctx.synchronize()
    for t in (sym, er):
        assert bool((t[0] == GUARD).all()) and bool((t[1 + T:] == GUARD).all()), "guard bands and unused slots are untouched"
    assert (blocks[T:] == -7).all() and closes[nf] == -7 and consumed[nf] == -7
    return closes[:nf], blocks[:T], sym[1:1 + T].cpu().numpy(), er[1:1 + T].cpu().numpy(), consumed[:nf]


def raw_flush(rx, flows):
    """ldpc_amd_fec_rxw_flows_flush_many into guarded buffers of nsel * W slots: (closes [nsel], blocks [T], sym [T], er [T])."""
    n, S, W = rx.n, rx.S, rx.window
    sel = None if flows is None else np.ascontiguousarray(flows, dtype=np.int32)
    nsel = rx.nflows if sel is None else len(sel)
    slots = nsel * W
    sym = torch.full((slots + 2, n, S), GUARD, dtype=torch.uint8, device="cuda")
    er = torch.full((slots + 2, n), GUARD, dtype=torch.uint8, device="cuda")
    blocks, closes = np.full(slots + 1, -7, dtype=np.int32), np.full(nsel + 1, -7, dtype=np.int32)
    T = rx._ctx._check(rx._L.ldpc_amd_fec_rxw_flows_flush_many(rx._h, None if sel is None else sel.ctypes.data, nsel, sym[1].data_ptr(),
                                                               er[1].data_ptr(), blocks.ctypes.data, closes.ctypes.data), "fec_rxw_flows_flush_many")
    rx._ctx.synchronize()
    for t in (sym, er):
        assert bool((t[0] == GUARD).all()) and bool((t[1 + T:] == GUARD).all()), "guard bands and unused slots are untouched"
    assert (blocks[T:] == -7).all() and closes[nsel] == -7
    return closes[:nsel], blocks[:T], sym[1:1 + T].cpu().numpy(), er[1:1 + T].cpu().numpy()


def same_flows(rx, hx, tag):
    for f in range(rx.nflows):
        assert rx.stats(f) == hx.stats(f) and rx.state(f) == hx.state(f) and rx.dropped(f) == hx.dropped(f), (tag, f)


def same_push(got, call, tag):
    closes, blocks, sym, er, consumed = got
    assert np.array_equal(closes, call.closes) and np.array_equal(consumed, call.consumed), tag
    assert np.array_equal(blocks, call.blocks), tag
    assert np.array_equal(sym, call.sym) and np.array_equal(er, call.er), tag


def same_flush(rx, hx, flows, tag):
    want = hx.flush_many(flows)
    got = raw_flush(rx, flows)
    for a, b in zip(got, want):
        assert np.array_equal(a, b), tag
    return int(got[0].sum())


# ------------------------------------------------------------------------------------------------------ 1. lockstep
@pytest.mark.parametrize("W,A", fc.LOCKSTEP_WA)
@pytest.mark.parametrize("nflows", fc.LOCKSTEP_NFLOWS)
def test_lockstep_with_host_objects(ctx, nflows, W, A):
    """Every flow against a host object of its own over calls cut at per-flow random sizes with max_blocks_per_flow from (1, 2, 64):
    after every call closes, blocks (slot order), bytes, flags, consumed, and per flow totals, state and dropped; then the flush."""
    streams = fc.lockstep_streams(nflows, A)
    ncalls = closed = 0
    with ctx.fec_rx_window_flows(nflows, N, K, rc.S, W, A) as rx, fc.HostFlows(nflows, W, A) as hx:
        for call in fc.lockstep_calls(hx, streams, fc.lockstep_seed(nflows, W, A)):
            pk, fb = fc.concat(call.pieces)
            tag = (nflows, W, A, ncalls, call.mb)
            same_push(raw_push(rx, dev(pk), fb, call.mb), call, tag)
            same_flows(rx, hx, tag)
            ncalls += 1
            closed += int(call.closes.sum())
        assert rx.pending().blocks == sum(hx.pending())
        closed += same_flush(rx, hx, None, "flush")
        same_flows(rx, hx, "flush")
        assert same_flush(rx, hx, None, "second flush") == 0
    assert closed >= 3 * nflows and ncalls >= 8   # (the two-buffer case W = 2, A = 0 loses the blocks behind an outage: few closes)


# ------------------------------------------------------------------------------------------------------ 2. the anchor
def test_window_2_is_the_multi_flow_receiver(ctx):
    """W = 2, A = 0: the same calls through FecRxFlows.push_many give the same closes, blocks, bytes, flags and consumed."""
    nflows = 3
    streams = fc.lockstep_streams(nflows, 0)
    total = 0
    with ctx.fec_rx_window_flows(nflows, N, K, rc.S, 2, 0) as rx, ctx.fec_rx_flows(nflows, N, K, rc.S) as old, fc.HostFlows(nflows, 2, 0) as hx:
        for i, call in enumerate(fc.lockstep_calls(hx, streams, 77)):
            pk, fb = fc.concat(call.pieces)
            d_pk = dev(pk)
            c1, b1, s1, e1, u1 = rx.push_many(d_pk, fb, call.mb)
            c0, b0, s0, e0, u0 = old.push_many(d_pk, fb, call.mb)
            assert np.array_equal(c0, c1) and np.array_equal(b0, b1) and np.array_equal(u0, u1), i
            assert torch.equal(s0, s1) and torch.equal(e0, e1), i
            assert np.array_equal(c1, call.closes) and np.array_equal(u1, call.consumed), i
            assert [rx.dropped(f) for f in range(nflows)] == old.dropped.tolist(), i
            total += int(c1.sum())
    assert total >= 9


# ------------------------------------------------------------------------------------------------------ 3. data paths
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("S", [1, 20, 16, 1024])
def test_data_paths(ctx, S, odd):
    """The 16-byte path (S % 16 == 0, aligned) and the byte path (any other S, or a packet array at an odd address); blocks carried in
    the staging planes from one call to a later one; duplicates with a flipped payload: the last copy wins."""
    nflows, W, A, mb = 3, 4, 10, 3
    streams = [rc.random_stream(rc.RANDOM_SEEDS[2 + f], S=S) for f in range(nflows)]
    hdr = [wm.headers(pk) for pk in streams]
    for pk, (blk, sym) in zip(streams, hdr):
        assert np.unique(np.stack([blk, sym]), axis=1).shape[1] < pk.shape[0], "the stream holds duplicates (their payload is flipped)"
    carried = 0
    with ctx.fec_rx_window_flows(nflows, N, K, S, W, A) as rx, fc.HostFlows(nflows, W, A, S_=S) as hx:
        for i, call in enumerate(fc.lockstep_calls(hx, streams, 5, sizes=(300, 17, 1111, 64, 2000), mbs=(mb,))):
            pk, fb = fc.concat(call.pieces, S)
            same_push(raw_push(rx, dev_at(pk, odd), fb, mb), call, (S, odd, i))
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


# ------------------------------------------------------------------------------------------------------ 4. decode
_CODES = {}


def get_code(ctx, which):
    key = (id(ctx), which)
    if key not in _CODES:
        if which == "rand":
            code = random_code()
            _CODES[key] = (ctx.register_code(code), code)
        else:
            _CODES[key] = (ctx.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which]), codes.load_builtin(which))
    return _CODES[key]


def coded_stream(ctx, h, code, S, F, seed, block0=0, loss=0.1, **link):
    """F random frames encoded and packetised on the device, thinned and sent through tools/link_model.py's link on the host:
    packets uint8 [P][8 + S] (numpy)."""
    src = torch.randint(0, 256, (F, code.k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    pk = ctx.fec_packetize_device(ctx.encode(h, src).view(F, code.n, S), 1, block0).cpu().numpy()
    keep = np.random.default_rng(seed + 1).random(pk.shape[0]) >= loss
    return rc.through_link(pk[keep], seed + 2, **link)


def to_host(fr, S):
    r = [x.cpu().numpy() for x in fr]
    r[0] = r[0].reshape(r[0].shape[0], r[4].shape[1], S)
    return r


def same_frames(got, want, tag):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (tag, name)


def decode_against_push(ctx, h, code, S, streams, W, A, mb=3, sizes=(700, 2500, 10 ** 9)):
    """Two objects over the same calls: one by decode_many / decode_flush_many, one by push_many / flush_many + Context.decode_frames.
    Everything the calls return must be equal.  Returns (blocks closed, the paths decode_many reported, the path of the flush)."""
    nf = len(streams)
    d_streams = [dev(pk) for pk in streams]
    pos, paths, closed, i = [0] * nf, set(), 0, 0
    with ctx.fec_rx_window_flows(nf, code.n, code.k, S, W, A) as rd, ctx.fec_rx_window_flows(nf, code.n, code.k, S, W, A) as rp:
        while any(pos[f] < streams[f].shape[0] for f in range(nf)):
            pieces = [d_streams[f][pos[f]:pos[f] + sizes[(i + f) % len(sizes)]] for f in range(nf)]
            fb = np.concatenate([[0], np.cumsum([p.shape[0] for p in pieces])]).astype(np.int64)
            d_pk = torch.cat(pieces)
            c1, b1, fr, u1 = rd.decode_many(h, d_pk, fb, mb)
            c0, b0, sym, er, u0 = rp.push_many(d_pk, fb, mb)
            assert np.array_equal(c0, c1) and np.array_equal(b0, b1) and np.array_equal(u0, u1) and u0.sum() > 0, i
            info = ctx.fec_rx_window_flows_info()
            assert info["blocks"] == len(b1)
            paths.add(info["path"])
            if len(b0):
                same_frames(to_host(fr, S), to_host(ctx.decode_frames(h, sym, er), S), ("decode_many", i))
                assert info["launches"] >= 1
            for f in range(nf):
                pos[f] += int(u0[f])
            closed += len(b0)
            i += 1
        order = list(range(nf))[::-1]
        assert rd.pending().blocks == rp.pending().blocks >= 1
        c1, b1, fr = rd.decode_flush_many(h, order)
        c0, b0, sym, er = rp.flush_many(order)
        assert np.array_equal(c0, c1) and np.array_equal(b0, b1) and len(b0) >= 1
        same_frames(to_host(fr, S), to_host(ctx.decode_frames(h, sym, er), S), "decode_flush_many")
        finfo = ctx.fec_rx_window_flows_info()
        assert finfo["blocks"] == len(b0)
        for f in range(nf):
            assert rd.stats(f) == rp.stats(f) and rd.state(f) == rp.state(f)
        assert rd.pending().blocks == 0
    return closed + len(b0), paths, finfo["path"]


def single_flow_path(ctx, h, code, S, pk, W, A):
    """The path FecRxWindow.decode_many reports for this code and S."""
    with ctx.fec_rx_window(code.n, code.k, S, W, A) as rx:
        rx.decode_many(h, dev(pk[:2500]), 3)
        return ctx.fec_rx_window_info()["path"]


@pytest.mark.parametrize("which,F", [("rand", 12), (1, 5)])
def test_decode_many_equals_push_many_and_decode_frames(ctx, which, F):
    """decode_many == push_many + decode_frames and decode_flush_many == flush_many + decode_frames, all six result arrays, fused and
    composed (the rx_pkt knob), and the info call reports fused exactly where FecRxWindow.decode_many does."""
    S, W, A, nf = 16, 4, 10, 3
    h, code = get_code(ctx, which)
    streams = [coded_stream(ctx, h, code, S, F, seed=400 + 10 * f + F, block0=(250 + 40 * f) & 0xFF, loss=0.10, window=code.n // 2, dup=0.02)
               for f in range(nf)]
    closed, paths, fpath = decode_against_push(ctx, h, code, S, streams, W, A)
    assert closed >= nf * (F - 1)
    want = single_flow_path(ctx, h, code, S, streams[0], W, A)
    assert paths == {want} and fpath == want
    if which == 1:
        assert want == "fused"
    ctx.configure("LDPC_AMD_RX_PKT", 0)
    try:
        closed0, paths0, fpath0 = decode_against_push(ctx, h, code, S, streams, W, A)
        info = ctx.fec_rx_window_flows_info()
        assert single_flow_path(ctx, h, code, S, streams[0], W, A) == "composed"
    finally:
        ctx.configure("LDPC_AMD_RX_PKT", None)
    assert closed0 == closed and paths0 == {"composed"} and fpath0 == "composed"
    assert info["launches"] >= 1 and 0 < info["scratch_bytes"] <= 256 << 20


def test_decode_word_sized_symbols():
    """S = 20 under symbol unit 4: decode_many takes the path FecRxWindow.decode_many takes; decode_flush_many is composed (S is no
    multiple of 16)."""
    S, W, A, nf, F = 20, 4, 10, 3, 8
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.set_symbol_unit(4)
        code = random_code()
        h = c.register_code(code)
        streams = [coded_stream(c, h, code, S, F, seed=500 + f, block0=10 * f, loss=0.10, window=100, dup=0.02) for f in range(nf)]
        closed, paths, fpath = decode_against_push(c, h, code, S, streams, W, A)
        assert closed >= nf * (F - 1) and fpath == "composed"
        assert paths == {single_flow_path(c, h, code, S, streams[0], W, A)}


# ------------------------------------------------------------------------------------------------------ 5. flush
def test_flush_many_of_a_subset(ctx):
    """A subset in non-ascending list order with a flow that has nothing open and a flow with an empty slot between two non-empty ones;
    the unlisted flow stays untouched and goes on in lockstep."""
    before, after = fc.flush_streams()
    nf, W, A = len(before), fc.FLUSH_W, fc.FLUSH_A
    with ctx.fec_rx_window_flows(nf, N, K, rc.S, W, A) as rx, fc.HostFlows(nf, W, A) as hx:
        for pieces in (before,):
            pk, fb = fc.concat(pieces)
            want = fc.Call(64, None, pieces, *hx.push_many(pieces, 64))
            same_push(raw_push(rx, dev(pk), fb, 64), want, "before")
        same_flows(rx, hx, "before")
        pend, hp = rx.pending(), hx.pending()
        assert pend.blocks == sum(hp) and hp[1] == 0 and hp[2] == 3
        for f in range(nf):
            assert pend.base[f] == hx.state(f)["base"] and pend.cnt[f].tolist() == hx.state(f)["cnt"]
        state3 = (rx.state(3), rx.stats(3))
        T = same_flush(rx, hx, fc.FLUSH_LIST, "subset")
        assert T == sum(hp[f] for f in fc.FLUSH_LIST), "pending() before the flush is what the flush closes"
        assert (rx.state(3), rx.stats(3)) == state3 and rx.pending().blocks == hp[3]
        same_flows(rx, hx, "after the flush")
        assert same_flush(rx, hx, fc.FLUSH_LIST, "second flush") == 0
        pk, fb = fc.concat(after)
        want = fc.Call(64, None, after, *hx.push_many(after, 64))
        same_push(raw_push(rx, dev(pk), fb, 64), want, "after")
        assert want.closes[3] >= 1
        same_flows(rx, hx, "after")
        assert same_flush(rx, hx, None, "the end") >= 3
        same_flows(rx, hx, "the end")


# ------------------------------------------------------------------------------------------------------ 6. the point of the feature
def test_an_outage_in_one_flow(ctx):
    """Flow 1's stream has one block at 50 %: the two-buffer rule never closes it and drops the rest of the flow; the window closes what
    its host object closes.  The healthy flows give the same blocks under both receivers."""
    W, A = 4, 10
    streams = [rc.packets_of(*rc.sent(40, lambda b: 0.95, 11), seed=1), rc.packets_of(*rc.outage_stream(), seed=2),
               rc.packets_of(*rc.sent(40, lambda b: 0.95, 13, block0=200), seed=3)]
    pk, fb = fc.concat(streams)
    d_pk = dev(pk)
    with ctx.fec_rx_window_flows(3, N, K, rc.S, W, A) as rx, ctx.fec_rx_flows(3, N, K, rc.S) as old, fc.HostFlows(3, W, A) as hx:
        want = fc.Call(64, None, streams, *hx.push_many(streams, 64))
        c1, b1, s1, e1, u1 = rx.push_many(d_pk, fb, 64)
        same_push((c1, b1, s1.cpu().numpy(), e1.cpu().numpy(), u1), want, "window")
        same_flows(rx, hx, "window")
        c0, b0, s0, e0, u0 = old.push_many(d_pk, fb, 64)
        assert c1[1] == want.closes[1] and c1[1] > c0[1], (c1.tolist(), c0.tolist())
        assert c1[1] >= 30 and c0[1] <= 5
        assert rx.dropped(1) < 100 < old.dropped[1]
        for f in (0, 2):
            new, prev = slice(int(c1[:f].sum()), int(c1[:f + 1].sum())), slice(int(c0[:f].sum()), int(c0[:f + 1].sum()))
            assert c1[f] == c0[f] >= 30 and np.array_equal(b1[new], b0[prev])
            assert torch.equal(s1[new], s0[prev]) and torch.equal(e1[new], e0[prev])


# ------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_are_atomic(ctx):
    L = ctx._L
    h = C.c_void_p()
    for args, text in [((0, N, K, 16, 4, 10), b"nflows"), ((4097, N, K, 16, 4, 10), b"nflows"), ((3, N, K, 16, 1, 10), b"window"),
                       ((3, N, K, 16, 33, 10), b"window"), ((3, N, K, 16, 4, -1), b"ahead_limit"), ((3, N, K, 16, 4, (1 << 30) + 1), b"ahead_limit"),
                       ((4096, 65536, K, 16, 32, 10), b"staging rows")]:
        assert L.ldpc_amd_fec_rxw_flows_create(ctx._h, *args, C.byref(h)) == EINVAL and text in L.ldpc_amd_last_error(ctx._h), args
    code_h, _ = get_code(ctx, "rand")   # (300, 200): not the object's (n, k)
    nf, W, A, mb = 3, 4, 10, 4
    streams = fc.lockstep_streams(nf, A)
    first = [pk[:1000] for pk in streams]
    rest = [pk[1000:] for pk in streams]
    with ctx.fec_rx_window_flows(nf, N, K, rc.S, W, A) as rx, fc.HostFlows(nf, W, A) as hx:
        pk, fb = fc.concat(first)
        want = fc.Call(64, None, first, *hx.push_many(first, 64))
        same_push(raw_push(rx, dev(pk), fb, 64), want, "first")
        before = [(rx.state(f), rx.stats(f)) for f in range(nf)]
        assert sum(sum(s["cnt"]) for s, _ in before) > 0
        pk, fb = fc.concat(rest)
        d_pk = dev(pk)
        slots = nf * mb
        sym = torch.empty((slots, N, rc.S), dtype=torch.uint8, device="cuda")
        er = torch.empty((slots, N), dtype=torch.uint8, device="cuda")
        out = torch.empty((max(slots, nf * W), 300, rc.S), dtype=torch.uint8, device="cuda")
        host = np.zeros((slots, N, rc.S), dtype=np.uint8)
        down = fb.copy()
        down[1], down[2] = fb[2], fb[1]
        assert down[2] < down[1]
        off = fb.copy()
        off[0] = 1
        twice = np.array([1, 1], dtype=np.int32)
        far = np.array([0, nf], dtype=np.int32)
        closes, used = np.zeros(nf, np.int32), np.zeros(nf, np.int64)

        def push(packets=d_pk.data_ptr(), begin=fb, s=sym.data_ptr(), e=er.data_ptr(), m=mb):
            return L.ldpc_amd_fec_rxw_flows_push_many(rx._h, packets, begin.ctypes.data if begin is not None else None, s, e, None,
                                                      closes.ctypes.data, m, used.ctypes.data)

        def decode(code=code_h, m=mb, o=out.data_ptr()):
            return L.ldpc_amd_fec_rxw_flows_decode_many(rx._h, code, d_pk.data_ptr(), fb.ctypes.data, 10, 1, o, None, None, None, None, None, None,
                                                        closes.ctypes.data, m, used.ctypes.data)

        def flush(sel, s=sym.data_ptr()):
            return L.ldpc_amd_fec_rxw_flows_flush_many(rx._h, sel.ctypes.data, len(sel), s, er.data_ptr(), None, None)

        refused = [(lambda: push(packets=pk.ctypes.data), b"device pointers"), (lambda: push(s=host.ctypes.data), b"device pointers"),
                   (lambda: push(begin=down), b"decreases"), (lambda: push(begin=off), b"start at 0"), (lambda: push(begin=None), b"flow_begin"),
                   (lambda: push(m=0), b"max_blocks_per_flow"), (lambda: push(m=(1 << 31) // (nf * N) + 1), b"2^31 - 2"),
                   (lambda: decode(), b"the code is (300,200)"), (lambda: decode(m=0), b"max_blocks_per_flow"),
                   (lambda: decode(code=code_h, o=host.ctypes.data), b"the code is"),
                   (lambda: flush(twice), b"twice"), (lambda: flush(far), b"no flow"), (lambda: flush(np.array([0], np.int32), s=host.ctypes.data), b"device pointers"),
                   (lambda: L.ldpc_amd_fec_rxw_flows_decode_flush_many(rx._h, code_h, twice.ctypes.data, 2, 10, 1, out.data_ptr(), None, None, None, None,
                                                                       None, None, None), b"twice"),
                   (lambda: L.ldpc_amd_fec_rxw_flows_decode_flush_many(rx._h, code_h, None, 0, 10, 1, out.data_ptr(), None, None, None, None, None,
                                                                       None, None), b"the code is")]
        for i, (call, text) in enumerate(refused):
            assert call() == EINVAL and text in L.ldpc_amd_last_error(ctx._h), (i, text, L.ldpc_amd_last_error(ctx._h))
            assert [(rx.state(f), rx.stats(f)) for f in range(nf)] == before, (i, text)
        assert rx.dropped(nf) == -1 and rx.dropped(-1) == -1
        want = fc.Call(mb, None, rest, *hx.push_many(rest, mb))
        same_push(raw_push(rx, d_pk, fb, mb), want, "the next good call")
        same_flows(rx, hx, "the next good call")
