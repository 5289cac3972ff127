"""GPU tests of the block-interleaved wire (include/ldpc_erasure_amd_interleave.h): the depth-D sender against the straight sender
placed by the layout, the grouped plan scan of the device receiver (csrc/rx_window_scan_dev.h) byte for byte against the C host
object -- which tests/test_interleave_cpu.py ties to the numpy model --, the data paths behind it, and sender -> link -> receiver on
the bursty channel.  Streams: tests/interleave_cases.py."""
import ctypes as C

import numpy as np
import pytest

import interleave_cases as ic
import rxw_cases as rc
from code_helpers import random_code
from ldpc_erasure_codes_amd import api, codes, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_rx_window import NAMES, oracle_frames, same_frames, to_host  # noqa: E402

wm, im = ic.wm, ic.im
N, K = ic.N, ic.K
EINVAL = -1
MIB = 1 << 20


class Variants:
    """One context per variant -- "default", "words" (symbol unit 4) -- and their code handles (1: built-in code 1, "rand":
    code_helpers.random_code(), (300,200))."""

    def __init__(self):
        self.ctx, self.codes = {}, {}

    def get(self, variant, which):
        if variant not in self.ctx:
            c = api.Context(0)
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            if variant == "words":
                c.set_symbol_unit(4)
            self.ctx[variant] = c
        c = self.ctx[variant]
        if (variant, which) not in self.codes:
            if which == "rand":
                code = random_code()
                self.codes[variant, which] = (c.register_code(code), code)
            else:
                self.codes[variant, which] = (c.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which]), codes.load_builtin(which))
        return (c,) + self.codes[variant, which]

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def variants():
    v = Variants()
    yield v
    v.close()


@pytest.fixture(scope="module")
def ctx(variants):
    return variants.get("default", "rand")[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_source(F, k, S, seed):
    src = torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    return src[:, :, 0].contiguous() if S == 1 else src


# ------------------------------------------------------------------------------------------------------ 1. the sender
# (variant, code, S, path): fused exactly where the multi-flow sender is
SENDER = [("default", 1, 128, "fused"), ("default", 1, 1024, "fused"), ("words", 1, 20, "fused"), ("default", "rand", 16, "composed"),
          ("default", 1, 1, "composed")]
F0, BLOCK0 = 11, 250   # a short first run, the 8-bit wrap, a short last run at every depth above 1


def wire_index(F, n, block0, D):
    frame, row = im.order(F, n, block0, D)
    return torch.from_numpy(frame * n + row).cuda()


def guarded(P, plen, guard=0xA5):
    """A packet array between two bands of 8 packets (8 * plen bytes keep the alignment of the allocation)."""
    buf = torch.full((P + 16, plen), guard, dtype=torch.uint8, device="cuda")
    return buf, buf[8:8 + P]


@pytest.mark.parametrize("variant,which,S,path", SENDER)
def test_sender_puts_every_packet_at_the_layouts_index(variants, variant, which, S, path):
    c, h, code = variants.get(variant, which)
    n = code.n
    src = make_source(F0, code.k, S, seed=40 + S)
    straight = c.fec_encode_packets_device(h, src, 7, BLOCK0)
    for D in ic.DEPTHS:
        buf, out = guarded(F0 * n, 8 + S)
        got = c.fec_encode_packets_interleaved_device(h, src, D, 7, BLOCK0, out=out)
        info = c.fec_sender_ilv_info()
        assert info["path"] == path and info["frames"] == F0 and info["descriptor_bytes"] >= 16 * F0
        assert info["scratch_bytes"] <= 256 * MIB and (path == "fused" or info["scratch_bytes"] > 0)
        assert torch.equal(got, straight.index_select(0, wire_index(F0, n, BLOCK0, D))), (S, D)
        assert bool((buf[:8] == 0xA5).all()) and bool((buf[-8:] == 0xA5).all()), "guard bands"
        first, stride = api.fec_tx_ilv_layout(F0, n, BLOCK0, D)
        f, j = F0 - 2, n - 1   # the contract, read literally, on one packet
        assert torch.equal(got[int(first[f]) + j * int(stride[f])], straight[f * n + j])
    assert torch.equal(c.fec_encode_packets_interleaved_device(h, src, 1, 7, BLOCK0), straight), "depth 1 is the straight sender"


def test_sender_fused_equals_composed(variants):
    c, h, code = variants.get("default", 1)
    S = 128
    src = make_source(F0, code.k, S, seed=5)
    fused = [c.fec_encode_packets_interleaved_device(h, src, D, 1, BLOCK0) for D in (4, 16)]
    assert c.fec_sender_ilv_info()["path"] == "fused"
    c.configure("LDPC_AMD_ENC_PKT", 0)
    try:
        composed = [c.fec_encode_packets_interleaved_device(h, src, D, 1, BLOCK0) for D in (4, 16)]
        info = c.fec_sender_ilv_info()
    finally:
        c.configure("LDPC_AMD_ENC_PKT", None)
    assert info["path"] == "composed" and 0 < info["scratch_bytes"] <= 256 * MIB
    for a, b in zip(fused, composed):
        assert torch.equal(a, b)
    c.fec_encode_packets_interleaved_device(h, src, 4, 1, BLOCK0)
    assert c.fec_sender_ilv_info()["path"] == "fused"


def test_sender_two_calls_back_to_back_and_the_flows_call_between(variants):
    """The descriptor staging is shared with the multi-flow sender: three calls enqueued without a synchronisation in between, each
    with another table, are all right, and each call reports through its own info."""
    c, h, code = variants.get("default", 1)
    n, S = code.n, 128
    a_src, b_src = make_source(9, code.k, S, seed=1), make_source(5, code.k, S, seed=2)
    want_a = c.fec_encode_packets_device(h, a_src, 1, 3).index_select(0, wire_index(9, n, 3, 8))
    want_b = c.fec_encode_packets_device(h, b_src, 2, 255).index_select(0, wire_index(5, n, 255, 2))
    c.synchronize()
    a = c.fec_encode_packets_interleaved_device(h, a_src, 8, 1, 3)
    fl = c.fec_encode_packets_flows_device(h, b_src, [0, 2, 5], 2, 255, api.TX_SEGMENTED)[0]
    b = c.fec_encode_packets_interleaved_device(h, b_src, 2, 2, 255)
    assert c.fec_sender_ilv_info()["frames"] == 5 and c.fec_sender_flows_info()["frames"] == 5
    c.synchronize()
    assert torch.equal(a, want_a) and torch.equal(b, want_b)
    assert torch.equal(fl[:2 * n], c.fec_encode_packets_device(h, b_src[:2], 2, 255))


def test_send_datagrams_trimmed_is_the_straight_senders_trim_placed_by_the_layout(variants):
    """FecTxInterleaved.send_datagrams_trimmed: the trim keys on each packet's own header, so datagram p of the interleaved wire is
    the straight sender's trimmed datagram of the packet the layout puts there; the block counter advances by the frames sent."""
    c, h, code = variants.get("default", 1)
    n, k, S, D = code.n, code.k, 128, 4
    rng = np.random.default_rng(3)
    lens = rng.integers(0, S - 3, size=3 * k - 7)   # 0 .. S - 4 bytes; the last frame is partly fillers
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    data = torch.randint(0, 256, (int(offsets[-1]),), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    tx, ref = c.fec_tx_interleaved(h, S, D, 1, 254), c.fec_tx_device(h, S, 1, 254)
    wire, want = tx.send_datagrams_trimmed(data, offsets), ref.send_datagrams_trimmed(data, offsets)
    assert tx.next_block == ref.next_block == (254 + 3) & 0xFF
    off, woff = wire.offset.cpu().numpy(), want.offset.cpu().numpy()
    idx = wire_index(3, n, 254, D).cpu().numpy()
    assert off.shape == woff.shape == (3 * n + 1,) and np.array_equal(np.diff(off), np.diff(woff)[idx])
    assert off[-1] == woff[-1] < 3 * n * (8 + S), "the same bytes in all, fewer than the untrimmed packets"
    got, exp = wire.bytes.cpu().numpy(), want.bytes.cpu().numpy()
    pos = np.concatenate([np.arange(woff[q], woff[q + 1]) for q in idx])
    assert np.array_equal(got[:off[-1]], exp[pos])


def test_sender_refusals_leave_the_context_usable(variants):
    c, h, code = variants.get("default", 1)
    L, n, k, S = c._L, code.n, code.k, 128
    src = make_source(3, k, S, seed=8)
    out = torch.empty((3 * n, 8 + S), dtype=torch.uint8, device="cuda")
    host = np.zeros((3 * n, 8 + S), dtype=np.uint8)

    def call(code_h=h, S_=S, F=3, s=src.data_ptr(), depth=4, o=out.data_ptr()):
        return L.ldpc_amd_fec_encode_packets_ilv_dev(c._h, code_h, S_, F, s, 1, 0, depth, o)

    for depth in (0, 3, 32, -4):
        assert call(depth=depth) == EINVAL and b"depth" in L.ldpc_amd_last_error(c._h)
    assert call(o=host.ctypes.data) == EINVAL and b"device pointers" in L.ldpc_amd_last_error(c._h)
    assert call(s=None) == EINVAL
    assert call(o=src.data_ptr()) == EINVAL and b"overlap" in L.ldpc_amd_last_error(c._h)
    assert call(F=-1) == EINVAL and call(F=(1 << 31) // n + 1) == EINVAL
    assert call(code_h=999) < 0 and call(S_=24) < 0, "an unknown code; S = 24 without word symbols"
    assert call(F=0, s=None, o=None) == 0, "no frames: nothing to do"
    info = (C.c_int64 * 4)()
    assert L.ldpc_amd_fec_sender_ilv_info(c._h, None) == EINVAL and L.ldpc_amd_fec_sender_ilv_info(c._h, info) == 0
    got = c.fec_encode_packets_interleaved_device(h, src, 4, 1, 0, out=out)
    assert torch.equal(got, c.fec_encode_packets_device(h, src, 1, 0).index_select(0, wire_index(3, n, 0, 4)))


# ------------------------------------------------------------------------------------------------------ 2. the grouped scan
def lockstep(ctx, pk, S, W, A, D, calls, n=N, k=K):
    """The device object and the host object, both of depth D, over the same calls [(start, end, max_blocks)]; a call that stops early
    is followed by calls over the rest of its piece.  Every call's blocks, bytes, flags, consumed, totals and state must agree; then
    the flushes."""
    d_pk = dev(pk)
    closed = 0
    with ctx.fec_rx_window(n, k, S, W, A, depth=D) as rx, api.FecRxWindowHost(n, k, S, W, A, depth=D) as hx:
        assert rx.depth == D == hx.depth
        for s, e, mb in calls:
            pos = s
            while True:
                hb, hs, he, hu = hx.push_many(pk[pos:e], mb)
                b, sy, er, u = rx.push_many(d_pk[pos:e], mb)
                tag = (W, A, D, s, e, mb, pos)
                assert u == hu and np.array_equal(b, hb), tag
                assert np.array_equal(sy.cpu().numpy(), hs) and np.array_equal(er.cpu().numpy(), he), tag
                assert rx.stats() == hx.stats() and rx.state() == hx.state() and rx.dropped == hx.dropped, tag
                closed += len(b)
                pos += u
                if pos >= e:
                    break
        hb, hs, he = hx.flush()
        b, sy, er = rx.flush()
        assert np.array_equal(b, hb) and np.array_equal(sy.cpu().numpy(), hs) and np.array_equal(er.cpu().numpy(), he)
        assert rx.stats() == hx.stats() and rx.state() == hx.state()
        assert len(rx.flush()[0]) == 0
        closed += len(b)
        totals = rx.stats()
    return closed, totals


@pytest.mark.parametrize("block0", ic.BLOCK0)
@pytest.mark.parametrize("W,D", ic.WD)
def test_scan_in_lockstep_with_the_host_object(ctx, W, D, block0):
    """The streams of tests/test_interleave_cpu.py -- all six per (W, D, block0): link window 0, 150 and 400, each without and with
    an ahead limit (thinned, reordered, duplicated with a flipped payload, foreign blocks, bad symbols; a thin group; an outage the
    window re-anchors behind) -- in calls of mixed sizes and small max_blocks."""
    resyncs = 0
    for A in ic.AHEAD:
        for i, lw in enumerate((0, 150, 400)):
            pk = ic.stream(1000 + 7 * D + i, D, block0, lw)
            edges = [0] + ic.small_cuts(pk.shape[0], 3 + i) + [pk.shape[0]]
            calls = [(s, e, (1, 2, 64)[j % 3]) for j, (s, e) in enumerate(zip(edges[:-1], edges[1:]))]
            closed, st = lockstep(ctx, pk, ic.S, W, A, D, calls)
            assert closed >= ic.frames_for(D) - 1 or A == 0, "(without an ahead limit the thin block stalls the window)"
            resyncs += st["resyncs"]
    assert resyncs >= 3, "every stream re-anchors behind its outage when there is an ahead limit"


def test_scan_plan_edges(ctx):
    """Events on lane 0, lane 63 and the last packet of a call; the 16 closes of a group's end on adjacent packets across a boundary of
    64 and across a call boundary; a g == 1 close and a re-anchor (into slot 5) inside one group of 64; a call of fewer than 64
    packets; the block number wrapping.  The facts are asserted from the model first."""
    calls = ic.edge_calls()
    facts = ic.edge_facts(calls)
    assert ic.EDGE_WANT <= facts, ic.EDGE_WANT - facts
    blk, sym = ic.edge_stream()
    pk = rc.packets_of(blk, sym)
    W, A, D = ic.EDGE_W, ic.EDGE_A, ic.EDGE_D
    many = [(s, e, 64) for s, e in calls]
    many.insert(3, (calls[3][0], calls[3][0], 1))   # npackets = 0 in the middle of the stream
    assert lockstep(ctx, pk, ic.S, W, A, D, many)[0] >= 64
    assert lockstep(ctx, pk, ic.S, W, A, D, [(0, pk.shape[0], 1)])[0] >= 64    # every close ends a call; the next continues mid-group
    assert lockstep(ctx, pk, ic.S, W, A, D, [(0, 3190, 5), (3190, pk.shape[0], 64)])[0] >= 64


@pytest.mark.parametrize("D,W", [(2, 4), (8, 16)])
def test_scan_keeps_every_row_of_a_loss_free_stream(ctx, D, W):
    """Fact (a) on the device: n rows per block, nothing late; the plain device object on the same wire drops packets as late."""
    blk, sym = ic.wire(24, 240, D)
    pk = rc.packets_of(blk, sym)
    d_pk = dev(pk)
    with ctx.fec_rx_window(N, K, ic.S, W, 10, depth=D) as rx:
        b, sy, er, u = rx.push_many(d_pk, 64)
        fb, fs, fe = rx.flush()
        flags = torch.cat([er, fe]).cpu().numpy()
        rows = N - flags.sum(axis=1)
        assert u == pk.shape[0] and rows[rows > 0].tolist() == [N] * 24 and rx.stats()["late"] == 0 and rx.dropped == 0
    with ctx.fec_rx_window(N, K, ic.S, W, 10) as rx:
        rx.push_many(d_pk, 64)
        assert rx.depth == 1 and rx.stats()["late"] > 300


# ------------------------------------------------------------------------------------------------------ 3. data paths
def interleaved_stream(c, h, code, S, F, D, seed, block0, loss=0.08, **link):
    """F random frames through the interleaved sender on the device, thinned and sent through tools/link_model.py's link on the host:
    packets uint8 [P][8 + S] (numpy)."""
    pk = c.fec_encode_packets_interleaved_device(h, make_source(F, code.k, S, seed), D, 1, block0).cpu().numpy()
    keep = np.random.default_rng(seed + 1).random(pk.shape[0]) >= loss
    return rc.through_link(pk[keep], seed + 2, **link)


def decode_stream(c, h, code, S, pk, W, A, D, how, sizes=(700, 2500, 10 ** 9), mb=3):
    """The whole stream through one FecRxWindow of depth D, call i made by how[i % len(how)] ("decode": decode_many, "push": push_many
    + decode_frames), the end by decode_flush or flush + decode_frames: (blocks, the six result arrays, paths seen, totals)."""
    d_pk = dev(pk)
    blocks, frames, paths = [], [], set()
    with c.fec_rx_window(code.n, code.k, S, W, A, depth=D) as rx:
        pos = i = 0
        while pos < pk.shape[0]:
            piece = d_pk[pos:pos + sizes[i % len(sizes)]]
            if how[i % len(how)] == "decode":
                b, fr, used = rx.decode_many(h, piece, mb)
                if len(b):
                    paths.add(c.fec_rx_window_info()["path"])
            else:
                b, sym, er, used = rx.push_many(piece, mb)
                fr = c.decode_frames(h, sym, er) if len(b) else None
            assert used > 0
            blocks += b.tolist()
            if len(b):
                frames.append(to_host(fr, S))
            pos += used
            i += 1
        if how[-1] == "decode":
            b, fr = rx.decode_flush(h)
        else:
            b, sym, er = rx.flush()
            fr = c.decode_frames(h, sym, er) if len(b) else None
        blocks += b.tolist()
        if len(b):
            frames.append(to_host(fr, S))
        stats = rx.stats()
    return blocks, [np.concatenate([f[j] for f in frames]) for j in range(6)], paths, stats


@pytest.mark.parametrize("variant,S", [("default", 1), ("default", 16), ("default", 1024), ("words", 20)])
def test_data_paths_decode_many_equals_push_many_and_decode_frames(variants, variant, S):
    """Every symbol length class behind the grouped scan: the byte path, the 16-byte path, word symbols; blocks carried from call to
    call in the staging planes; decode_flush."""
    c, h, code = variants.get(variant, "rand")
    F, D, W, A = 10, 4, 8, 10
    pk = interleaved_stream(c, h, code, S, F, D, seed=500 + S, block0=250, window=120, dup=0.02)
    ref_b, ref, _, ref_stats = decode_stream(c, h, code, S, pk, W, A, D, ("push",))
    sent = {(250 + f) & 0xFF for f in range(F)}
    assert sent <= set(ref_b) and (ref[3] <= 1).sum() >= F - 1, "the stream closes and decodes its blocks"
    b, fr, paths, stats = decode_stream(c, h, code, S, pk, W, A, D, ("decode",))
    assert b == ref_b and stats == ref_stats and paths
    same_frames(fr, ref, "decode_many")
    b, fr, _, stats = decode_stream(c, h, code, S, pk, W, A, D, ("decode", "push"), sizes=(333, 1500, 64))
    assert b == ref_b and stats == ref_stats
    same_frames(fr, ref, "mixed")


def test_data_paths_fused_equals_composed(variants):
    c, h, code = variants.get("default", 1)
    S, F, D, W, A = 16, 8, 4, 8, 10
    pk = interleaved_stream(c, h, code, S, F, D, seed=9, block0=252, window=code.n, dup=0.02)
    ref_b, ref, _, ref_stats = decode_stream(c, h, code, S, pk, W, A, D, ("push",), sizes=(5000, 9000, 10 ** 9))
    assert len(ref_b) >= F and (ref[3] <= 1).sum() >= F - 1
    b, fr, paths, stats = decode_stream(c, h, code, S, pk, W, A, D, ("decode",), sizes=(5000, 9000, 10 ** 9))
    assert paths == {"fused"} and b == ref_b and stats == ref_stats
    same_frames(fr, ref, "fused")
    c.configure("LDPC_AMD_RX_PKT", 0)
    try:
        b, fr, paths0, stats = decode_stream(c, h, code, S, pk, W, A, D, ("decode",), sizes=(5000, 9000, 10 ** 9))
    finally:
        c.configure("LDPC_AMD_RX_PKT", None)
    assert paths0 == {"composed"} and b == ref_b and stats == ref_stats
    same_frames(fr, ref, "composed")


def test_receiver_refusals_are_atomic(ctx):
    L = ctx._L
    h = C.c_void_p()
    for depth in (0, 3, 32):
        assert L.ldpc_amd_fec_rxw_dev_create_depth(ctx._h, N, K, 16, 32, 10, depth, C.byref(h)) == EINVAL
        assert b"depth" in L.ldpc_amd_last_error(ctx._h)
    for W, D in [(3, 2), (7, 4), (31, 16), (16, 16)]:
        assert L.ldpc_amd_fec_rxw_dev_create_depth(ctx._h, N, K, 16, W, 10, D, C.byref(h)) == EINVAL
        assert b"2 * depth <= window" in L.ldpc_amd_last_error(ctx._h)
        with pytest.raises(api.LdpcAmdError):
            ctx.fec_rx_window(N, K, 16, W, 10, depth=D)
    assert L.ldpc_amd_fec_rxw_dev_create_depth(ctx._h, N, K, 16, 33, 10, 4, C.byref(h)) == EINVAL and b"window" in L.ldpc_amd_last_error(ctx._h)
    W, A, D = 8, 10, 4
    pk = ic.stream(31, D, 250, 150)
    d_pk = dev(pk)
    with ctx.fec_rx_window(N, K, ic.S, W, A, depth=D) as rx, api.FecRxWindowHost(N, K, ic.S, W, A, depth=D) as hx:
        rx.push_many(d_pk[:1000], 64)
        hx.push_many(pk[:1000], 64)
        before = (rx.state(), rx.stats())
        sym = torch.empty((4, N, ic.S), dtype=torch.uint8, device="cuda")
        er = torch.empty((4, N), dtype=torch.uint8, device="cuda")
        host = np.zeros((4, N, ic.S), dtype=np.uint8)
        used = C.c_int64(0)
        rest = d_pk[1000:]

        def push(packets=rest.data_ptr(), np_=rest.shape[0], s=sym.data_ptr(), e=er.data_ptr(), mb=4):
            return L.ldpc_amd_fec_rxw_dev_push_many(rx._h, packets, np_, s, e, None, mb, C.byref(used))

        for call, text in [(lambda: push(packets=pk.ctypes.data), b"device pointers"), (lambda: push(s=host.ctypes.data), b"device pointers"),
                           (lambda: push(mb=0), b"max_blocks"), (lambda: push(np_=1 << 31), b"npackets")]:
            assert call() == EINVAL and text in L.ldpc_amd_last_error(ctx._h), text
            assert (rx.state(), rx.stats()) == before
        hb, hs, he, hu = hx.push_many(pk[1000:], 64)
        b, sy, e2, u = rx.push_many(rest, 64)
        assert u == hu and np.array_equal(b, hb) and np.array_equal(sy.cpu().numpy(), hs) and np.array_equal(e2.cpu().numpy(), he)
        assert rx.state() == hx.state() and rx.stats() == hx.stats()


# ------------------------------------------------------------------------------------------------------ 4. end to end
E2E_F, E2E_BLOCK0, E2E_W, E2E_A = 32, 248, 16, 10


def pipeline(ctx, oc, h, code, src, D, lost, **link):
    """sender (depth D) -> FecLink -> FecRxWindow(depth D): (source blocks recovered on the device, on the host + oracle)."""
    S = src.shape[2]
    tx = ctx.fec_tx_interleaved(h, S, D, 1, E2E_BLOCK0) if D > 1 else ctx.fec_tx_device(h, S, 1, E2E_BLOCK0)
    pk = tx.send(src)
    assert tx.next_block == (E2E_BLOCK0 + E2E_F) & 0xFF
    arrived = ctx.fec_link(seed=5, **link).send(pk, lost=lost)[0]
    pk_host = arrived.cpu().numpy()
    with ctx.fec_rx_window(code.n, code.k, S, E2E_W, E2E_A, depth=D) as rx:
        b, fr, used = rx.decode_many(h, arrived, 64)
        assert used == arrived.shape[0]
        fb, ffr = rx.decode_flush(h)
        got_b = b.tolist() + fb.tolist()
        parts = [to_host(x, S) for x, y in ((fr, b), (ffr, fb)) if len(y)]
        got = [np.concatenate([p[j] for p in parts]) for j in range(6)]
        stats = rx.stats()
    with api.FecRxWindowHost(code.n, code.k, S, E2E_W, E2E_A, depth=D) as hx:
        hb, hs, he, hu = hx.push_many(pk_host, 64)
        fb, fs, fe = hx.flush()
        assert hx.stats() == stats
    hb, hs, he = hb.tolist() + fb.tolist(), np.concatenate([hs, fs]), np.concatenate([he, fe])
    assert got_b == hb
    out, sw, res, st = oracle_frames(oc, hs, he)
    for name, a, w in zip(NAMES[:4], got[:4], (out, sw, res, st)):
        assert np.array_equal(a, w), name
    src_host = src.cpu().numpy()

    def recovered(frames, blocks):
        return sum(int(np.array_equal(frames[j, :code.k], src_host[(bn - E2E_BLOCK0) & 0xFF])) for j, bn in enumerate(blocks)
                   if (bn - E2E_BLOCK0) & 0xFF < E2E_F)

    return recovered(got[0], got_b), recovered(out, hb)


def test_end_to_end_interleaving_recovers_what_the_bursts_take(ctx, variants, oracle):
    """FecTxInterleaved(8) -> FecLink (no reordering, the Gilbert-Elliott loss flags of seed 79) -> FecRxWindow(W = 16, A = 10,
    depth 8) on the (300,200) code: 32 of 32 source blocks come back; the depth-1 pipeline on the same flags recovers fewer (30,
    tests/test_interleave_cpu.py::test_burst_table).  A second run with reordering and duplicates: device == host + oracle."""
    S = 16
    _, h, code = variants.get("default", "rand")
    oc = oracle.OracleCode(code)
    src = make_source(E2E_F, code.k, S, seed=9)
    lost = dev(synth.erasures_bursty(79, 0, E2E_F * code.n, 1, 0.13, 0.8, 10.0).reshape(-1))
    deep = pipeline(ctx, oc, h, code, src, 8, lost, window=0)
    assert deep == (E2E_F, E2E_F)
    flat = pipeline(ctx, oc, h, code, src, 1, lost, window=0)
    assert flat[0] == flat[1] < E2E_F
    dev_n, host_n = pipeline(ctx, oc, h, code, src, 8, lost, window=1000, dup=0.02, dup_flip=True)
    assert dev_n == host_n
