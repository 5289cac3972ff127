"""GPU tests of the windowed receiver on the device (include/ldpc_erasure_amd_rx_window.h, csrc/rx_window_dev.hip).  Every comparison
is byte for byte against the C host object (api.FecRxWindowHost), which tests/test_rx_window_cpu.py ties to the numpy model; decoded
frames are compared with Context.decode_frames on the host object's blocks and with the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import rxw_cases as rc
from code_helpers import random_code
from ldpc_erasure_codes_amd import api, codes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

wm = rc.wm
N, K = rc.N, rc.K
EINVAL = -1
NAMES = ("out", "sweeps", "residual", "status", "erased_out", "residual_src")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def lockstep(ctx, pk, S, W, A, calls, n=N, k=K, end=True):
    """The device object and the host object over the same calls [(start, end, max_blocks)]; a call that stops early is followed by
    calls over the rest of its piece.  Every call's blocks, bytes, flags, consumed, totals and state must agree; then the flushes."""
    d_pk = dev(pk)
    closed = 0
    with ctx.fec_rx_window(n, k, S, W, A) as rx, api.FecRxWindowHost(n, k, S, W, A) as hx:
        for s, e, mb in calls:
            pos = s
            while True:
                hb, hs, he, hu = hx.push_many(pk[pos:e], mb)
                b, sy, er, u = rx.push_many(d_pk[pos:e], mb)
                tag = (W, A, s, e, mb, pos)
                assert u == hu and np.array_equal(b, hb), tag
                assert np.array_equal(sy.cpu().numpy(), hs) and np.array_equal(er.cpu().numpy(), he), tag
                assert rx.stats() == hx.stats() and rx.state() == hx.state() and rx.dropped == hx.dropped, tag
                closed += len(b)
                pos += u
                if pos >= e:
                    break
        if end:
            hb, hs, he = hx.flush()
            b, sy, er = rx.flush()
            assert np.array_equal(b, hb) and np.array_equal(sy.cpu().numpy(), hs) and np.array_equal(er.cpu().numpy(), he)
            assert rx.stats() == hx.stats() and rx.state() == hx.state()
            assert len(rx.flush()[0]) == 0
            closed += len(b)
    return closed


# ------------------------------------------------------------------------------------------------------ 1. plan edges
@pytest.mark.parametrize("A", rc.EDGE_A)
@pytest.mark.parametrize("W", rc.EDGE_W)
def test_plan_edges(ctx, W, A):
    """Events on lane 0, lane 63 and the last packet of a call, two closes and a close + re-anchor inside one group of 64, a call of
    fewer than 64 packets, npackets = 0, max_blocks = 1 stopping mid-group, the block number wrapping
    (tests/test_rx_window_cpu.py::test_plan_edge_stream_places_its_events asserts that the stream does all that)."""
    blk, sym = rc.edge_stream(A)
    pk = rc.packets_of(blk, sym)
    calls = rc.edge_calls(blk, sym, W, A)
    many = [(s, e, 64) for s, e in calls]
    many.insert(3, (calls[3][0], calls[3][0], 1))   # npackets = 0 in the middle of the stream
    assert lockstep(ctx, pk, rc.S, W, A, many) >= 9
    assert lockstep(ctx, pk, rc.S, W, A, [(0, pk.shape[0], 1)]) >= 9    # every close ends a call; the next continues mid-group
    assert lockstep(ctx, pk, rc.S, W, A, [(0, 777, 2), (777, pk.shape[0], 3)]) >= 9


@pytest.mark.parametrize("W,A", [(2, 0), (4, 10), (8, 3), (32, 1)])
def test_random_streams_in_mixed_calls(ctx, W, A):
    for seed in (rc.RANDOM_SEEDS[1], "wrap"):
        pk = rc.random_stream(**rc.WRAP) if seed == "wrap" else rc.random_stream(seed)
        rng = np.random.default_rng(7)
        calls, pos = [], 0
        while pos < pk.shape[0]:
            c = int(rng.choice([1, 17, 63, 64, 65, 300, 1111]))
            calls.append((pos, min(pos + c, pk.shape[0]), int(rng.choice([1, 2, 64]))))
            pos += c
        lockstep(ctx, pk, rc.S, W, A, calls)


# ------------------------------------------------------------------------------------------------------ 2. data paths
def raw_push(rx, d_pk, mb, S, guard=0xA5):
    """ldpc_amd_fec_rxw_dev_push_many into the middle of guarded buffers: (blocks, sym [mb], er [mb], used); asserts the bands."""
    sym = torch.full((mb + 2, N, S), guard, dtype=torch.uint8, device="cuda")
    er = torch.full((mb + 2, N), guard, dtype=torch.uint8, device="cuda")
    blocks = np.zeros(mb, dtype=np.int32)
    used = C.c_int64(0)
    nb = rx._ctx._check(rx._L.ldpc_amd_fec_rxw_dev_push_many(rx._h, d_pk.data_ptr(), d_pk.shape[0], sym[1].data_ptr(), er[1].data_ptr(),
                                                             blocks.ctypes.data, mb, C.byref(used)), "push_many")
    rx._ctx.synchronize()
    for t in (sym, er):
        assert bool((t[0] == guard).all()) and bool((t[1 + nb:] == guard).all()), "guard bands and unused slots are untouched"
    return blocks[:nb], sym[1:1 + nb].cpu().numpy(), er[1:1 + nb].cpu().numpy(), used.value


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("S", [1, 20, 16, 1024])
def test_data_paths(ctx, S, odd):
    """The 16-byte path (S % 16 == 0, aligned) and the byte path (any other S, or a packet array at an odd address); carried blocks
    read from the staging planes by a later call; duplicates with another payload; guard bands."""
    pk = rc.random_stream(rc.RANDOM_SEEDS[2], S=S)
    P = pk.shape[0]
    buf = torch.zeros(P * (8 + S) + 16, dtype=torch.uint8, device="cuda")
    off = 1 if odd else 0
    d_pk = buf[off:off + P * (8 + S)].view(P, 8 + S)
    d_pk.copy_(dev(pk))
    assert d_pk.data_ptr() % 2 == off
    blk, sym = wm.headers(pk)
    assert np.unique(np.stack([blk, sym]), axis=1).shape[1] < P, "the stream holds duplicates (their payload is flipped)"
    carried = 0
    W, A, mb = 4, 10, 3
    with ctx.fec_rx_window(N, K, S, W, A) as rx, api.FecRxWindowHost(N, K, S, W, A) as hx:
        pos = 0
        for c in [300, 17, 1111, 64, 5000]:
            e = min(pos + c, P)
            while pos < e:
                hb, hs, he, hu = hx.push_many(pk[pos:e], mb)
                b, sy, er, u = raw_push(rx, d_pk[pos:e], mb, S)
                assert u == hu and np.array_equal(b, hb) and np.array_equal(sy, hs) and np.array_equal(er, he), (S, odd, pos)
                here = [np.unique(sym[pos:pos + u][(blk[pos:pos + u] == bn) & (sym[pos:pos + u] < N)]).size for bn in b]
                carried += sum(int(N - he[j].sum() > here[j]) for j in range(len(b)))
                pos += u
        assert carried >= 3, "closed blocks that hold rows an earlier call received"
        hb, hs, he = hx.flush()
        b, sy, er = rx.flush()
        assert len(hb) >= 1 and np.array_equal(b, hb) and np.array_equal(sy.cpu().numpy(), hs) and np.array_equal(er.cpu().numpy(), he)
        assert rx.stats() == hx.stats() and rx.state() == hx.state()


# ------------------------------------------------------------------------------------------------------ 3. decode
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
    r[0] = r[0].reshape(r[0].shape[0], r[4].shape[1], S)   # (also for no frames at all)
    return r


def same_frames(got, want, tag):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (tag, name)


def two_calls(ctx, rx, h, S, d_pk, mb):
    """push_many + Context.decode_frames: what decode_many fuses."""
    b, sym, er, used = rx.push_many(d_pk, mb)
    fr = ctx.decode_frames(h, sym, er) if len(b) else None
    return b, (to_host(fr, S) if len(b) else None), used


def decode_stream(ctx, h, code, S, pk, W, A, how, sizes=(700, 2500, 10 ** 9), mb=3):
    """The whole stream through one FecRxWindow, call i made by how[i % len(how)] ("decode": decode_many, "push": push_many +
    decode_frames), the end by decode_flush or flush + decode_frames: (blocks, the six result arrays concatenated, paths seen)."""
    d_pk = dev(pk)
    blocks, frames, paths = [], [], set()
    with ctx.fec_rx_window(code.n, code.k, S, W, A) as rx:
        pos = i = 0
        while pos < pk.shape[0]:
            piece = d_pk[pos:pos + sizes[i % len(sizes)]]
            kind = how[i % len(how)]
            if kind == "decode":
                b, fr, used = rx.decode_many(h, piece, mb)
                fr = to_host(fr, S) if len(b) else None
                if len(b):
                    paths.add(ctx.fec_rx_window_info()["path"])
                    assert ctx.fec_rx_window_info()["blocks"] == len(b)
            else:
                b, fr, used = two_calls(ctx, rx, h, S, piece, mb)
            assert used > 0
            blocks += b.tolist()
            if len(b):
                frames.append(fr)
            pos += used
            i += 1
        if how[-1] == "decode":
            b, fr = rx.decode_flush(h)
            fr = to_host(fr, S) if len(b) else None
        else:
            b, sym, er = rx.flush()
            fr = to_host(ctx.decode_frames(h, sym, er), S) if len(b) else None
        blocks += b.tolist()
        if len(b):
            frames.append(fr)
        stats = rx.stats()
    return blocks, [np.concatenate([f[j] for f in frames]) for j in range(6)], paths, stats


@pytest.mark.parametrize("which,F", [("rand", 12), (1, 5)])
def test_decode_many_equals_push_many_and_decode_frames(ctx, which, F):
    """decode_many == push_many + decode_frames, fused == composed, decode_flush == flush + decode_frames, any mix of the calls gives
    the same bytes, and the info call names the path."""
    S = 16
    h, code = get_code(ctx, which)
    pk = coded_stream(ctx, h, code, S, F, seed=300 + F, block0=253, loss=0.08, window=code.n // 2, dup=0.02)
    W, A = 4, 10
    ref_b, ref, _, ref_stats = decode_stream(ctx, h, code, S, pk, W, A, ("push",))
    assert len(ref_b) >= F - 1 and (ref[3] <= 1).sum() >= F - 2, "the stream closes and decodes its blocks"
    b, fr, paths, stats = decode_stream(ctx, h, code, S, pk, W, A, ("decode",))
    assert b == ref_b and stats == ref_stats
    same_frames(fr, ref, "decode_many")
    if which == 1:
        assert paths == {"fused"}
    ctx.configure("LDPC_AMD_RX_PKT", 0)
    try:
        b, fr, paths0, stats = decode_stream(ctx, h, code, S, pk, W, A, ("decode",))
        info = ctx.fec_rx_window_info()
    finally:
        ctx.configure("LDPC_AMD_RX_PKT", None)
    assert paths0 == {"composed"} and info["path"] == "composed" and info["launches"] >= 1 and 0 < info["scratch_bytes"] <= 256 << 20
    assert b == ref_b and stats == ref_stats
    same_frames(fr, ref, "composed")
    for how in [("decode", "push"), ("push", "decode", "decode")]:
        b, fr, _, stats = decode_stream(ctx, h, code, S, pk, W, A, how, sizes=(333, 1500, 64))
        assert b == ref_b and stats == ref_stats
        same_frames(fr, ref, how)


def oracle_frames(oc, sym, er):
    """out / sweeps / residual / status of the blocks sym [B][n][S], er [B][n] from the CPU oracle."""
    B = sym.shape[0]
    out = np.zeros_like(sym)
    _, sw, res, st = oc.decode_batch_s1(np.zeros(er.shape, dtype=np.uint8), er, itenum=10, do_ml=1)
    for f in range(B):
        out[f], _, sw[f], info, _ = oc.decode_packets(sym[f], er[f], itenum=10, do_ml=1)
        res[f] = info[0]
    return out, sw, res, st


def test_end_to_end_sender_link_receiver(ctx, oracle):
    """sender -> FecLink (window 1000, Gilbert-Elliott loss, dup 0.02) -> FecRxWindow(W = 8) on the (300,200) code: the decoded blocks
    are the host object's blocks decoded by the oracle, and as many source blocks are fully recovered as on the host side."""
    S, F = 16, 24
    h, code = get_code(ctx, "rand")
    oc = oracle.OracleCode(code)
    src = torch.randint(0, 256, (F, code.k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    tx = ctx.fec_tx_device(h, S, 1, 250)
    pk = tx.send(src)
    from ldpc_erasure_codes_amd import synth
    lost = dev(synth.erasures_bursty(77, 0, pk.shape[0], 1, 0.13, 0.8, 10.0).reshape(-1))
    link = ctx.fec_link(seed=5, window=1000, dup=0.02, dup_flip=True)
    arrived = link.send(pk, lost=lost)
    arrived = arrived[0] if isinstance(arrived, tuple) else arrived
    pk_host = arrived.cpu().numpy()
    W, A = 8, 10
    with ctx.fec_rx_window(code.n, code.k, S, W, A) as rx:
        b, fr, used = rx.decode_many(h, arrived, 64)
        assert used == arrived.shape[0]
        fb, ffr = rx.decode_flush(h)
        got_b = b.tolist() + fb.tolist()
        got = [np.concatenate([x, y]) for x, y in zip(to_host(fr, S), to_host(ffr, S))]
        stats = rx.stats()
    with api.FecRxWindowHost(code.n, code.k, S, W, A) as hx:
        hb, hs, he, hu = hx.push_many(pk_host, 64)
        fb, fs, fe = hx.flush()
        assert hx.stats() == stats
    hb, hs, he = hb.tolist() + fb.tolist(), np.concatenate([hs, fs]), np.concatenate([he, fe])
    assert got_b == hb and len(hb) >= F - 2
    out, sw, res, st = oracle_frames(oc, hs, he)
    for name, a, w in zip(NAMES[:4], got[:4], (out, sw, res, st)):
        assert np.array_equal(a, w), name
    src_host = src.cpu().numpy()
    first = 250
    recovered_dev = sum(int(np.array_equal(got[0][j, :code.k], src_host[(bn - first) & 0xFF])) for j, bn in enumerate(got_b) if (bn - first) & 0xFF < F)
    recovered_host = sum(int(np.array_equal(out[j, :code.k], src_host[(bn - first) & 0xFF])) for j, bn in enumerate(hb) if (bn - first) & 0xFF < F)
    assert recovered_dev == recovered_host and recovered_host >= 1


# ------------------------------------------------------------------------------------------------------ 4. the anchor
@pytest.mark.parametrize("which,F", [("rand", 10)])
def test_anchor_on_the_device(ctx, which, F):
    """W = 2, A = 0 returns what FecRxDevice.decode_many returns on the same packets."""
    S = 16
    h, code = get_code(ctx, which)
    pk = coded_stream(ctx, h, code, S, F, seed=77, loss=0.05, window=40, dup=0.02, bad_sym=0.01, foreign=0.01)
    d_pk = dev(pk)
    with ctx.fec_rx_window(code.n, code.k, S, 2, 0) as rx, ctx.fec_rx_device(code.n, code.k, S) as old:
        pos = 0
        total = 0
        for c in [500, 64, 1200, 10 ** 9]:
            piece = d_pk[pos:pos + c]
            while piece.shape[0]:
                b0, f0, u0 = old.decode_many(h, piece, 2)
                b1, f1, u1 = rx.decode_many(h, piece, 2)
                assert u0 == u1 and np.array_equal(b0, b1) and rx.dropped == old.dropped
                if len(b0):
                    same_frames(to_host(f1, S), to_host(f0, S), pos)
                total += len(b0)
                pos += u0
                piece = piece[u0:]
        assert total >= F - 2
        st = rx.stats()
        assert st["ahead_total"] == 0 and st["resyncs"] == 0 and st["bad_symbol"] > 0 and st["late"] > 0


# ------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_are_atomic(ctx):
    L = ctx._L
    h = C.c_void_p()
    code_h, _ = get_code(ctx, "rand")
    for W, A in [(1, 0), (33, 0), (4, -1)]:
        assert L.ldpc_amd_fec_rxw_dev_create(ctx._h, N, K, 16, W, A, C.byref(h)) == EINVAL
        assert b"window" in L.ldpc_amd_last_error(ctx._h)
    pk = rc.random_stream(rc.RANDOM_SEEDS[0])
    d_pk = dev(pk)
    with ctx.fec_rx_window(N, K, rc.S, 4, 10) as rx, api.FecRxWindowHost(N, K, rc.S, 4, 10) as hx:
        rx.push_many(d_pk[:1000], 64)
        hx.push_many(pk[:1000], 64)
        before = (rx.state(), rx.stats())
        sym = torch.empty((4, N, rc.S), dtype=torch.uint8, device="cuda")
        er = torch.empty((4, N), dtype=torch.uint8, device="cuda")
        host = np.zeros((4, N, rc.S), dtype=np.uint8)
        used = C.c_int64(0)
        rest = d_pk[1000:]

        def push(packets=rest.data_ptr(), np_=rest.shape[0], s=sym.data_ptr(), e=er.data_ptr(), mb=4):
            return L.ldpc_amd_fec_rxw_dev_push_many(rx._h, packets, np_, s, e, None, mb, C.byref(used))

        refused = [(lambda: push(packets=pk.ctypes.data), b"device pointers"), (lambda: push(s=host.ctypes.data), b"device pointers"),
                   (lambda: push(mb=0), b"max_blocks"), (lambda: push(np_=1 << 31), b"npackets"), (lambda: push(np_=-1), b"npackets"),
                   (lambda: L.ldpc_amd_fec_rxw_dev_flush(rx._h, host.ctypes.data, er.data_ptr(), None), b"device pointers"),
                   (lambda: L.ldpc_amd_fec_rxw_dev_decode_many(rx._h, code_h, rest.data_ptr(), rest.shape[0], 10, 1, sym.data_ptr(), None, None,
                                                               None, None, None, None, 0, C.byref(used)), b"max_blocks")]
        for call, text in refused:
            assert call() == EINVAL and text in L.ldpc_amd_last_error(ctx._h), text
            assert (rx.state(), rx.stats()) == before
        hb, hs, he, hu = hx.push_many(pk[1000:], 64)
        b, sy, e2, u = rx.push_many(rest, 64)
        assert u == hu and np.array_equal(b, hb) and np.array_equal(sy.cpu().numpy(), hs) and np.array_equal(e2.cpu().numpy(), he)
        assert rx.state() == hx.state() and rx.stats() == hx.stats()
