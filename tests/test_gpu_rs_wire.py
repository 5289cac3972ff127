"""GPU tests of Reed-Solomon on the FEC wire (include/ldpc_erasure_amd_rs_wire.h).  Every expectation is an equality against code
paths that exist without the feature, or against the oracle: the sender's packets against Context.rs_encode ->
Context.fec_packetize_device placed by the interleaver's layout; the receiver's RS calls against the C host receiver followed by
Context.rs_decode_frames and by the oracle's decoder on the first k received symbols; sender -> link -> receiver against
tools/rs_wire_model.py.  Streams: tests/rs_wire_cases.py."""
import ctypes as C

import numpy as np
import pytest

import interleave_cases as ic
import rs_wire_cases as rw
from ldpc_erasure_codes_amd import api, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

rm, wm, im, lm = rw.rm, rw.wm, rw.im, rw.rc.lm
EINVAL, ENOCODE, EUNSUP = -1, -4, -5
MIB = 1 << 20
B0, BLOCK0 = 11, 250   # a short first run, the 8-bit wrap, a short last run at depth 8 and 16
DEPTHS = (1, 8, 16)


class Contexts:
    """One context per variant -- "default", "words" (symbol unit 4) -- and their RS handles."""

    def __init__(self):
        self.ctx, self.rs = {}, {}

    def get(self, variant, n, k):
        if variant not in self.ctx:
            c = api.Context(0)
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            if variant == "words":
                c.set_symbol_unit(4)
            self.ctx[variant] = c
        c = self.ctx[variant]
        if (variant, n, k) not in self.rs:
            self.rs[variant, n, k] = c.rs_create(n, k)
        return c, self.rs[variant, n, k]

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def contexts():
    v = Contexts()
    yield v
    v.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_source(B, k, S, seed):
    src = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    return src[:, :, 0].contiguous() if S == 1 else src


def wire_index(B, n, block0, D):
    frame, row = im.order(B, n, block0, D)
    return torch.from_numpy(frame * n + row).cuda()


def composition(c, rs, n, k, src, fec_class, block0, D):
    """What the parent commit offers: rs_encode, fec_packetize_device, and the layout applied by a gather."""
    cw = c.rs_encode(rs, n, k, src)
    straight = c.fec_packetize_device(cw if cw.ndim == 3 else cw.unsqueeze(-1).contiguous(), fec_class, block0)
    return straight.index_select(0, wire_index(src.shape[0], n, block0, D))


def guarded(P, plen, guard=0xA5, shift=0):
    """A packet array between two bands of 8 packets, `shift` bytes off the alignment of the allocation."""
    buf = torch.full(((P + 16) * plen + 8,), guard, dtype=torch.uint8, device="cuda")
    body = buf[shift:shift + (P + 16) * plen].view(P + 16, plen)
    return buf, body[8:8 + P], shift + 8 * plen, shift + (8 + P) * plen


def guards_intact(buf, lo, hi, guard=0xA5):
    return bool((buf[:lo] == guard).all()) and bool((buf[hi:] == guard).all())


# ------------------------------------------------------------------------------------------------------ 1. the sender's bytes
# R = 32 a full group of accumulators; R = 63 not a multiple of 4, above 32; R = 1; k and R below one group; R = 37 > k
CODES = [(255, 223), (255, 192), (255, 254), (12, 5), (40, 3)]
# S = 16 one short slice with idle lanes; 272 a full slice and a 16-byte tail; 1024 four slices; 1 always composed
SYMBOLS = [("default", 16, "fused"), ("default", 272, "fused"), ("default", 1024, "fused"), ("default", 1, "composed"),
           ("words", 20, "fused"), ("words", 1460, "fused")]


@pytest.mark.parametrize("n,k", CODES)
def test_sender_bytes_equal_rs_encode_and_packetize_placed_by_the_layout(contexts, n, k):
    for variant, S, path in SYMBOLS:
        c, rs = contexts.get(variant, n, k)
        src = make_source(B0, k, S, seed=n + k + S)
        for D in DEPTHS:
            want = composition(c, rs, n, k, src, api.FEC_CLASS_RS, BLOCK0, D)
            buf, out, lo, hi = guarded(B0 * n, 8 + S)
            got = c.fec_rs_encode_packets_device(rs, src, D, block0=BLOCK0, out=out)
            info = c.fec_rs_sender_info()
            assert info["path"] == path and info["blocks"] == B0 and info["descriptor_bytes"] >= 16 * B0, (S, D, info)
            assert info["scratch_bytes"] <= 256 * MIB and (path == "fused" or info["scratch_bytes"] > 0)
            assert torch.equal(got, want), (variant, S, D)
            assert guards_intact(buf, lo, hi), "guard bands"
            first, stride = api.fec_tx_ilv_layout(B0, n, BLOCK0, D)
            b, j = B0 - 2, n - 1   # the contract, read literally, on one packet
            straight = composition(c, rs, n, k, src, api.FEC_CLASS_RS, BLOCK0, 1)
            assert torch.equal(got[int(first[b]) + j * int(stride[b])], straight[b * n + j])


def test_sender_against_the_oracle(contexts):
    n, k, S, D = 40, 3, 16, 8
    c, rs = contexts.get("default", n, k)
    src = make_source(B0, k, S, seed=3)
    got = c.fec_rs_encode_packets_device(rs, src, D, block0=BLOCK0).cpu().numpy()
    assert c.fec_rs_sender_info()["path"] == "fused"
    assert np.array_equal(c.rs_generator(rs, n, k), rw.generator(n, k))
    assert np.array_equal(got, rm.send(rw.generator(n, k), src.cpu().numpy(), BLOCK0, D))


def test_sender_composed_paths_give_the_fused_bytes(contexts):
    """ENC_PKT = 0, and a packet array 4 bytes off an 8-byte boundary: composed, the same bytes."""
    n, k, S = 255, 192, 272
    c, rs = contexts.get("default", n, k)
    src = make_source(B0, k, S, seed=5)
    fused = [c.fec_rs_encode_packets_device(rs, src, D, block0=BLOCK0) for D in (1, 8)]
    assert c.fec_rs_sender_info()["path"] == "fused"
    c.configure("LDPC_AMD_ENC_PKT", 0)
    try:
        composed = [c.fec_rs_encode_packets_device(rs, src, D, block0=BLOCK0) for D in (1, 8)]
        info = c.fec_rs_sender_info()
    finally:
        c.configure("LDPC_AMD_ENC_PKT", None)
    assert info["path"] == "composed" and 0 < info["scratch_bytes"] <= 256 * MIB
    for a, b in zip(fused, composed):
        assert torch.equal(a, b)
    buf, out, lo, hi = guarded(B0 * n, 8 + S, shift=4)
    assert out.data_ptr() % 8 == 4
    got = c.fec_rs_encode_packets_device(rs, src, 8, block0=BLOCK0, out=out)
    assert c.fec_rs_sender_info()["path"] == "composed" and torch.equal(got, fused[1]) and guards_intact(buf, lo, hi)
    c.fec_rs_encode_packets_device(rs, src, 8, block0=BLOCK0)
    assert c.fec_rs_sender_info()["path"] == "fused"


def test_sender_more_items_than_wavefronts(contexts):
    """(12,5), S = 16: one (block, slice) item per block.  The launch holds at most 20 wavefronts per compute unit, 5120 on 256 of
    them: 6000 blocks make the wavefronts stride over the items."""
    n, k, S, B = 12, 5, 16, 6000
    c, rs = contexts.get("default", n, k)
    src = make_source(B, k, S, seed=6)
    for D in (1, 16):
        got = c.fec_rs_encode_packets_device(rs, src, D, block0=BLOCK0)
        info = c.fec_rs_sender_info()
        assert info["path"] == "fused" and info["blocks"] == B
        assert torch.equal(got, composition(c, rs, n, k, src, api.FEC_CLASS_RS, BLOCK0, D))


def test_sender_no_blocks_and_two_calls_back_to_back(contexts):
    n, k, S = 255, 223, 272
    c, rs = contexts.get("default", n, k)
    before = c.fec_rs_sender_info()
    buf, out, lo, hi = guarded(0, 8 + S)
    empty = torch.empty((0, k, S), dtype=torch.uint8, device="cuda")
    assert c._L.ldpc_amd_fec_rs_encode_packets_dev(c._h, rs, S, 0, None, 2, 0, 8, None) == 0
    assert c.fec_rs_encode_packets_device(rs, empty, 8, out=out).shape == (0, 8 + S) and guards_intact(buf, lo, hi)
    assert c.fec_rs_sender_info() == before, "no blocks: nothing to report"
    a_src, b_src = make_source(9, k, S, seed=1), make_source(5, k, S, seed=2)
    want_a = composition(c, rs, n, k, a_src, 2, 3, 8)
    want_b = composition(c, rs, n, k, b_src, 9, 255, 2)
    c.synchronize()
    a = c.fec_rs_encode_packets_device(rs, a_src, 8, 2, 3)
    b = c.fec_rs_encode_packets_device(rs, b_src, 2, 9, 255)   # enqueued behind it: another table in the same device memory
    assert c.fec_rs_sender_info()["blocks"] == 5
    c.synchronize()
    assert torch.equal(a, want_a) and torch.equal(b, want_b)


# ------------------------------------------------------------------------------------------------------ 2. refusals
def test_sender_refusals_leave_the_context_usable_and_packets_untouched(contexts):
    n, k, S = 255, 192, 64
    c, rs = contexts.get("default", n, k)
    L = c._L
    src = make_source(3, k, S, seed=8)
    buf, out, lo, hi = guarded(3 * n, 8 + S)
    host = np.zeros((3 * n, 8 + S), dtype=np.uint8)

    def call(rs_=rs, S_=S, B=3, s=src.data_ptr(), depth=8, o=out.data_ptr()):
        return L.ldpc_amd_fec_rs_encode_packets_dev(c._h, rs_, S_, B, s, 2, 0, depth, o)

    def err():
        return L.ldpc_amd_last_error(c._h)

    want = composition(c, rs, n, k, src, api.FEC_CLASS_RS, 0, 8)
    refused = [(dict(rs_=999), ENOCODE, b"RS handle"), (dict(rs_=-1), ENOCODE, b"RS handle"),
               (dict(B=(1 << 31) // n + 1), EINVAL, b"2^31"), (dict(B=-1), EINVAL, b"nblocks"),
               (dict(depth=0), EINVAL, b"depth"), (dict(depth=3), EINVAL, b"depth"), (dict(depth=32), EINVAL, b"depth"), (dict(depth=-4), EINVAL, b"depth"),
               (dict(o=host.ctypes.data), EINVAL, b"device pointers"), (dict(s=host.ctypes.data), EINVAL, b"device pointers"),
               (dict(s=None), EINVAL, b"device pointers"), (dict(o=None), EINVAL, b"device pointers"),
               (dict(o=src.data_ptr()), EINVAL, b"overlap"), (dict(S_=24), EUNSUP, b"S"), (dict(S_=0), EINVAL, b"S")]
    for kwargs, code, text in refused:
        assert call(**kwargs) == code and text in err(), kwargs
        c.synchronize()
        assert bool((buf == 0xA5).all()), ("a refused call writes nothing", kwargs)
        got = c.fec_rs_encode_packets_device(rs, src, 8, out=out)
        assert torch.equal(got, want) and guards_intact(buf, lo, hi), kwargs
        out.fill_(0xA5)
    info = (C.c_int64 * 4)()
    assert L.ldpc_amd_fec_rs_sender_info(c._h, None) == EINVAL and L.ldpc_amd_fec_rs_sender_info(c._h, info) == 0
    assert list(info)[0] == 1 and list(info)[3] == 3


# ------------------------------------------------------------------------------------------------------ 3. the receiver
def rs_frames(c, rs, k, S):
    """decode(sym, er) of rs_wire_cases.host_reference: Context.rs_decode_frames on the planes the host receiver handed out, and
    beside it the oracle's decoder on the first k received symbols."""
    g = c.rs_generator(rs, *c.rs_info(rs))

    def decode(sym, er):
        if sym.shape[0] == 0:
            return np.zeros((0, k, S), np.uint8), np.zeros(0, np.int32), np.zeros(0, np.int32)
        r = c.rs_decode_frames(rs, sym, er)
        o = rm.decode_planes(g, sym, er)
        for a, b in zip(r, o):
            assert np.array_equal(a, b), "Context.rs_decode_frames against the oracle"
        return r.msg, r.received, r.status

    return decode


def same_call(got, want, what):
    blocks, msg, received, status = got[:4]
    assert blocks.tolist() == want["blocks"], what
    for name, a, w in zip(("msg", "received", "status"), (msg, received, status), want["dec"]):
        assert np.array_equal(a.cpu().numpy(), w), (what, name)


@pytest.mark.parametrize("W,A,D", rw.WAD)
@pytest.mark.parametrize("k", [192, 223])
def test_rs_decode_many_equals_host_push_many_and_rs_decode_frames(contexts, k, W, A, D):
    n, S = 255, rw.S
    c, rs = contexts.get("default", n, k)
    B1, B2 = rw.nblocks_for(D)
    src = make_source(B1 + B2, k, S, seed=k + D)
    parts = rw.pieces(lambda f, cnt, b0: c.fec_rs_encode_packets_device(rs, src[f:f + cnt], D, block0=b0).cpu().numpy(), n, k, D, seed=k + 7 * D)
    assert c.fec_rs_sender_info()["path"] == "fused", "the payloads are the new sender's"
    model = rw.model_blocks(parts, n, k, W, A, D)
    assert rw.facts([x for piece in model for half in piece for x in half], n, k) == rw.WANT
    assert any(len(win) == 0 for piece in model for _, win in piece[0]) == (A > 0 and D > 1), "an empty leading slot leaves by the ahead limit"
    decode = rs_frames(c, rs, k, S)
    for max_blocks in (1, 3, 1 << 10):
        cuts = [ic.small_cuts(pk.shape[0], seed=max_blocks + j) for j, pk in enumerate(parts)]
        want = rw.host_reference(decode, parts, n, k, W, A, D, cuts, max_blocks)
        with c.fec_rx_window(n, k, S, W, A, depth=D) as rx:
            for (pk, cut), (calls, flush), piece in zip(zip(parts, cuts), want, model):
                d_pk = dev(pk)
                edges = [0] + cut + [pk.shape[0]]
                it = iter(calls)
                handed = []
                for s, e in zip(edges[:-1], edges[1:]):
                    pos = s
                    while pos < e:
                        w_ = next(it)
                        got = rx.rs_decode_many(rs, d_pk[pos:e], max_blocks)
                        same_call(got, w_, (max_blocks, pos))
                        assert got[4] == w_["used"] and rx.stats() == w_["stats"] and rx.state() == w_["state"], (max_blocks, pos)
                        assert c.fec_rs_receiver_info()["blocks"] == len(w_["blocks"]) or not len(w_["blocks"])
                        handed += w_["blocks"]
                        pos += got[4]
                assert next(it, None) is None and handed == [b for b, _ in piece[0]]
                got = rx.rs_decode_flush(rs)
                same_call(got, flush, (max_blocks, "flush"))
                assert rx.stats() == flush["stats"] and rx.state() == flush["state"] and flush["blocks"] == [b for b, _ in piece[1]]
                info = c.fec_rs_receiver_info()
                assert info["blocks"] == len(flush["blocks"]) and info["launches"] >= 1 and 0 < info["scratch_bytes"] <= 256 * MIB


def test_erased_batch_and_a_plain_push_many_behind_an_rs_call(contexts):
    """The erased_batch output is push_many's; push_many, the RS call and the flushes continue one another on one object."""
    n, k, S, (W, A, D) = 255, 192, rw.S, rw.WAD[1]
    c, rs = contexts.get("default", n, k)
    B1, B2 = rw.nblocks_for(D)
    src = make_source(B1 + B2, k, S, seed=77)
    pk = rw.pieces(lambda f, cnt, b0: c.fec_rs_encode_packets_device(rs, src[f:f + cnt], D, block0=b0).cpu().numpy(), n, k, D, seed=78)[0]
    half = pk.shape[0] // 2
    d_pk = dev(pk)
    with api.FecRxWindowHost(n, k, S, W, A, depth=D) as hx, c.fec_rx_window(n, k, S, W, A, depth=D) as rx:
        hb, hs, he, hu = hx.push_many(pk[:half], 64)
        assert len(hb) > 0, "the first call closes blocks"
        msg = torch.empty((64, k, S), dtype=torch.uint8, device="cuda")
        er = torch.full((64, n), 7, dtype=torch.uint8, device="cuda")
        blocks = np.zeros(64, dtype=np.int32)
        used = C.c_int64(0)
        nb = c._L.ldpc_amd_fec_rxw_dev_rs_decode_many(rx._h, rs, d_pk.data_ptr(), half, msg.data_ptr(), None, None, er.data_ptr(), blocks.ctypes.data,
                                                      64, C.byref(used))
        assert nb == len(hb) and used.value == hu and blocks[:nb].tolist() == hb.tolist()
        assert np.array_equal(er[:nb].cpu().numpy(), he) and bool((er[nb:] == 7).all())
        assert np.array_equal(msg[:nb].cpu().numpy(), c.rs_decode_frames(rs, hs, he).msg)
        # a plain push_many continues from the same state, and an RS flush ends it
        hb2, hs2, he2, hu2 = hx.push_many(pk[half:], 64)
        b2, s2, e2, u2 = rx.push_many(d_pk[half:], 64)
        assert b2.tolist() == hb2.tolist() and u2 == hu2 and np.array_equal(s2.cpu().numpy(), hs2) and np.array_equal(e2.cpu().numpy(), he2)
        assert rx.stats() == hx.stats() and rx.state() == hx.state()
        fb, fs, fe = hx.flush()
        gb, gm, gr, gs = rx.rs_decode_flush(rs)
        ref = c.rs_decode_frames(rs, fs, fe)
        assert gb.tolist() == fb.tolist() and np.array_equal(gm.cpu().numpy(), ref.msg) and np.array_equal(gr.cpu().numpy(), ref.received)
        assert np.array_equal(gs.cpu().numpy(), ref.status) and rx.stats() == hx.stats() and rx.state() == hx.state()
        assert rx.rs_decode_flush(rs)[0].shape == (0,), "nothing left"


def test_receiver_for_another_code_is_refused_and_left_unchanged(contexts):
    n, k, S = 255, 192, rw.S
    c, rs = contexts.get("default", n, k)
    _, other = contexts.get("default", 255, 223)
    src = make_source(2, k, S, seed=9)
    pk = c.fec_rs_encode_packets_device(rs, src, 1, block0=0)
    with c.fec_rx_window(n, k, S, 4, 10) as rx:
        assert rx.rs_decode_many(rs, pk[:200], 4)[0].shape == (0,)
        state, stats = rx.state(), rx.stats()
        for bad, code in ((other, EINVAL), (999, ENOCODE)):
            with pytest.raises(api.LdpcAmdError):
                rx.rs_decode_many(bad, pk[200:], 4)
            with pytest.raises(api.LdpcAmdError):
                rx.rs_decode_flush(bad)
            assert rx.state() == state and rx.stats() == stats
        host = np.zeros((4, k, S), dtype=np.uint8)
        used = C.c_int64(0)
        assert c._L.ldpc_amd_fec_rxw_dev_rs_decode_many(rx._h, rs, pk[200:].data_ptr(), 310, host.ctypes.data, None, None, None, None, 4,
                                                        C.byref(used)) == EINVAL
        assert c._L.ldpc_amd_fec_rxw_dev_rs_decode_many(rx._h, rs, pk[200:].data_ptr(), 310, None, None, None, None, None, 0, C.byref(used)) == EINVAL
        assert rx.state() == state and rx.stats() == stats
        b, msg, received, status, used = rx.rs_decode_many(rs, pk[200:], 4)
        assert b.tolist() == [0, 1] and torch.equal(msg, src) and received.tolist() == [n, n] and status.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------ 4. end to end on the device
def test_sender_link_receiver_on_the_bursty_channel_equals_the_model(contexts):
    n, k, S, D, B = 255, 192, rw.S, 8, 40
    c, rs = contexts.get("default", n, k)
    src = make_source(B, k, S, seed=12)
    tx = c.fec_tx_rs(rs, S, depth=D, block0=0)
    pk = tx.send(src)
    assert tx.next_block == B and c.fec_rs_sender_info()["path"] == "fused"
    lost = dev(synth.erasures_bursty(79, 0, B * n, 1, 0.13, 0.8, 10.0).reshape(-1))   # the cfg 3 channel, one draw per wire position
    arrived, _, l_src, l_fate = c.fec_link(seed=5, window=120, dup_flip=True).send(pk, lost=lost)
    a_host = lm.apply(pk.cpu().numpy(), l_src.cpu().numpy(), l_fate.cpu().numpy().view(np.uint16))[0]
    assert np.array_equal(a_host, arrived.cpu().numpy()) and 0 < arrived.shape[0] < B * n
    with c.fec_rx_window(n, k, S, 16, 10, depth=D) as rx:
        b1, m1, r1, s1, used = rx.rs_decode_many(rs, arrived, 64)
        assert used == arrived.shape[0]
        b2, m2, r2, s2 = rx.rs_decode_flush(rs)
        stats = rx.stats()
    blocks = b1.tolist() + b2.tolist()
    msg = torch.cat([m1, m2]).cpu().numpy()
    received, status = torch.cat([r1, r2]).tolist(), torch.cat([s1, s2]).tolist()
    closed, flushed, win = rm.receive(rw.generator(n, k), a_host, 16, 10, D)
    want = closed + flushed
    assert (blocks, received, status) == ([x.number for x in want], [x.received for x in want], [x.status for x in want])
    assert stats == win.totals and [x.number for x in closed] == b1.tolist()
    src_host = src.cpu().numpy()
    decoded = [j for j, st in enumerate(status) if st == 0]
    assert len(decoded) > B // 2, "most blocks survive the channel at depth 8"
    for j in decoded:
        assert blocks[j] < B and np.array_equal(msg[j], src_host[blocks[j]]), blocks[j]
        assert np.array_equal(msg[j], want[j].msg)
