"""GPU tests of the Reed-Solomon decoder on rows in place (include/ldpc_erasure_amd_rs_rows.h) and of the windowed receiver's fused RS
call built on it.  Every expectation is an equality: the decoder against Context.rs_decode_frames on the frames the source words
describe and against tools/rs_rows_model.py; the fused receiver against the composed one (knob RX_PKT = 0) and against the C host
receiver followed by Context.rs_decode_frames.  Blocks: tests/rs_rows_cases.py; streams: tests/rs_wire_cases.py."""
import ctypes as C

import numpy as np
import pytest

import interleave_cases as ic
import rs_rows_cases as rc
import rs_wire_cases as rw
from ldpc_erasure_codes_amd import api

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

rr = rc.rr
EINVAL, ENOCODE, EUNSUP = -1, -4, -5
GUARD, BAND = 0xA5, 4096   # the fill of everything a call must leave alone, and the bytes of it on either side of an array
WAVES = 4                  # wavefronts per workgroup of the stream kernel, and its workgroups per compute unit
WGS_PER_CU = 5


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


def banded(a, shift=0):
    """The array `a` on the device between two bands of GUARD, `shift` bytes behind a 16-byte boundary: (buffer, view of a, lo, hi)."""
    a = np.ascontiguousarray(a)
    buf = torch.full((BAND + shift + a.nbytes + BAND,), GUARD, dtype=torch.uint8, device="cuda")
    lo, hi = BAND + shift, BAND + shift + a.nbytes
    buf[lo:hi] = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
    return buf, buf[lo:hi].view(a.shape) if a.dtype == np.uint8 else buf[lo:hi].view(torch.int32).view(a.shape), lo, hi


def bands_intact(buf, lo, hi):
    return bool((buf[:lo] == GUARD).all()) and bool((buf[hi:] == GUARD).all())


def outputs(B, n, k, S, extra=2):
    """msg with `extra` rows of blocks behind it, received, status, erased_out: all at GUARD."""
    msg = torch.full((B + extra, k, S), GUARD, dtype=torch.uint8, device="cuda")
    received, status = (torch.full((B + extra,), -1515870811, dtype=torch.int32, device="cuda") for _ in range(2))
    er = torch.full((B + extra, n), GUARD, dtype=torch.uint8, device="cuda")
    return msg, received, status, er


def untouched(outs):
    msg, received, status, er = outs
    return bool((msg == GUARD).all()) and bool((er == GUARD).all()) and bool((received == -1515870811).all()) and bool((status == -1515870811).all())


# ------------------------------------------------------------------------------------------------------ 1. the decoder over the case list
# S = 16 one slice with 60 idle lanes; 256 one full slice; 272 two overlapping slices; 1024 four; 20 only under symbol unit 4
SYMBOLS = [("default", 16), ("default", 256), ("default", 272), ("default", 1024), ("words", 20)]


@pytest.mark.parametrize("variant,S", SYMBOLS)
@pytest.mark.parametrize("n,k", rc.CODES)
def test_rs_decode_rows_equals_rs_decode_frames_and_the_model(contexts, n, k, variant, S):
    c, rs = contexts.get(variant, n, k)
    g = c.rs_generator(rs, n, k)
    cs = rc.cases(n, k)
    if len(cs) % WAVES == 0:
        cs = cs + [cs[1]]
    order = np.random.default_rng(S).permutation(len(cs))   # neighbouring wavefronts hold different r
    cs = [cs[i] for i in order]
    B = len(cs)
    assert B % WAVES != 0
    built = rc.build(cs, n, k, S, seed=n + k + S)
    assert rc.facts(cs, built, n, k) >= rc.want(n, k)
    pbuf, d_pk, plo, phi = banded(built.packets, shift=8)
    sbuf, d_st, slo, shi = banded(built.stage)
    wbuf, d_src, wlo, whi = banded(built.src.view(np.int32))
    assert d_pk.data_ptr() % 16 == 8, "8-byte but not 16-byte aligned"
    outs = outputs(B, n, k, S)
    msg, received, status, er = outs
    got = c.rs_decode_rows(rs, d_src, d_pk, d_st, out=(msg[:B], received[:B], status[:B]), erased_out=er[:B])
    c.synchronize()
    sym, flags = rr.frames(built.src, built.packets, built.stage)
    ref = c.rs_decode_frames(rs, dev(sym), dev(flags))
    model = rr.decode_rows(g, built.src, built.packets, built.stage)
    for name, a, b, m in zip(("msg", "received", "status"), got, ref, model):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), (name, "against rs_decode_frames")
        assert np.array_equal(a.cpu().numpy(), m), (name, "against the model")
    assert np.array_equal(er[:B].cpu().numpy(), flags) and np.array_equal(flags, model[3])
    assert bool((msg[B:] == GUARD).all()) and bool((er[B:] == GUARD).all()) and bool((received[B:] == -1515870811).all())
    assert bands_intact(pbuf, plo, phi) and bands_intact(sbuf, slo, shi) and bands_intact(wbuf, wlo, whi)
    assert np.array_equal(d_pk.cpu().numpy(), built.packets) and np.array_equal(d_st.cpu().numpy(), built.stage), "the rows are read only"
    # the rows behind the first k of a block do not matter; the optional outputs may be left out
    other = rc.build(cs, n, k, S, seed=n + k + S, garbage=5)
    again = c.rs_decode_rows(rs, dev(other.src.view(np.int32)), dev(other.packets), dev(other.stage))
    assert torch.equal(again.msg, msg[:B]) and torch.equal(again.received, received[:B]) and torch.equal(again.status, status[:B])
    m2 = torch.full((B, k, S), GUARD, dtype=torch.uint8, device="cuda")
    assert c._L.ldpc_amd_rs_decode_rows_dev(c._h, rs, S, B, d_src.data_ptr(), d_pk.data_ptr(), d_pk.shape[0], d_st.data_ptr(), d_st.shape[0],
                                            m2.data_ptr(), None, None, None) == 0
    assert torch.equal(m2, msg[:B])


def test_rs_decode_rows_from_packets_alone_and_from_staging_rows_alone(contexts):
    """packets == NULL with a count of 0, and stage == NULL with a count of 0."""
    n, k, S = 15, 11, 64
    c, rs = contexts.get("default", n, k)
    rng = np.random.default_rng(4)
    rows = rng.integers(0, 256, size=(3 * n, 8 + S), dtype=np.uint8)
    words = rng.permutation(3 * n).astype(np.uint32).reshape(3, n)
    words[0, [1, 12]] = rr.ROW_ERASED
    words[2, :5] = rr.ROW_ERASED   # short
    sym, flags = rr.frames(words, rows, None)
    ref = c.rs_decode_frames(rs, dev(sym), dev(flags))
    from_packets = c.rs_decode_rows(rs, dev(words.view(np.int32)), packets=dev(rows))
    from_stage = c.rs_decode_rows(rs, dev((words | rr.ROW_STAGED).view(np.int32)), stage=dev(rows[:, 8:]))
    assert ref.status.tolist() == [0, 0, 1]
    for got in (from_packets, from_stage):
        assert all(torch.equal(a, b) for a, b in zip(got, ref))


# ------------------------------------------------------------------------------------------------------ 2. the persistent grid strides
def test_more_items_than_wavefronts_of_the_grid(contexts):
    """(15,11), S = 1024: four (block, slice) items per block.  The launch holds at most WGS_PER_CU workgroups of WAVES wavefronts per
    compute unit: a few blocks more than fill them make the wavefronts stride over the items."""
    n, k, S = 15, 11, 1024
    c, rs = contexts.get("default", n, k)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slices = (S + 255) // 256
    B = cus * WGS_PER_CU * WAVES // slices + 7
    assert B * slices > cus * WGS_PER_CU * WAVES
    gen = torch.Generator(device="cuda").manual_seed(11)
    packets = torch.randint(0, 256, (B * n, 8 + S), dtype=torch.uint8, device="cuda", generator=gen)
    lost = torch.rand((B, n), device="cuda", generator=gen) < 0.15
    words = torch.arange(B * n, dtype=torch.int32, device="cuda").view(B, n).masked_fill(lost, -1)
    got = c.rs_decode_rows(rs, words, packets=packets)
    ref = c.rs_decode_frames(rs, packets[:, 8:].reshape(B, n, S).contiguous(), lost.to(torch.uint8))
    assert 0 < int(ref.status.sum()) < B // 4, "some blocks are short, most are not"
    assert all(torch.equal(a, b) for a, b in zip(got, ref))


# ------------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_leave_the_outputs_alone_and_the_context_usable(contexts):
    n, k, S, B = 255, 192, 64, 3
    c, rs = contexts.get("default", n, k)
    _, deep = contexts.get("default", 255, 128)
    L = c._L
    rng = np.random.default_rng(2)
    rows = rng.integers(0, 256, size=(B * n + 1, 8 + S), dtype=np.uint8)
    words = rng.permutation(B * n).astype(np.uint32).reshape(B, n)
    words[:, 3:40] = rr.ROW_ERASED
    d_rows, d_words = dev(rows), dev(words.view(np.int32))
    sym, flags = rr.frames(words, rows, None)
    want = c.rs_decode_frames(rs, dev(sym), dev(flags))
    outs = outputs(B, n, k, S, extra=0)
    msg, received, status, er = outs
    host = np.zeros((B, k, S), dtype=np.uint8)
    flat = d_rows.view(-1)

    def call(rs_=rs, S_=S, B_=B, src=d_words.data_ptr(), pk=d_rows.data_ptr(), npk=B * n, m=msg.data_ptr()):
        return L.ldpc_amd_rs_decode_rows_dev(c._h, rs_, S_, B_, src, pk, npk, None, 0, m, received.data_ptr(), status.data_ptr(), er.data_ptr())

    refused = [(dict(S_=1), EUNSUP), (dict(rs_=deep), EUNSUP), (dict(pk=flat[4:].data_ptr()), EUNSUP), (dict(S_=24), EUNSUP),
               (dict(m=flat[S:].data_ptr()), EINVAL), (dict(m=host.ctypes.data), EINVAL), (dict(src=words.ctypes.data), EINVAL),
               (dict(m=None), EINVAL), (dict(src=None), EINVAL), (dict(pk=None), EINVAL), (dict(npk=-1), EINVAL), (dict(B_=-1), EINVAL),
               (dict(B_=(1 << 31) // n + 1), EINVAL), (dict(m=d_words.data_ptr()), EINVAL), (dict(rs_=999), ENOCODE), (dict(rs_=-1), ENOCODE)]
    before = d_rows.clone()
    for kwargs, code in refused:
        assert call(**kwargs) == code and L.ldpc_amd_last_error(c._h), kwargs
        c.synchronize()
        assert untouched(outs) and torch.equal(d_rows, before), ("a refused call writes nothing", kwargs)
        assert call() == 0, kwargs
        c.synchronize()
        assert torch.equal(msg, want.msg) and torch.equal(received, want.received) and torch.equal(status, want.status), kwargs
        assert np.array_equal(er.cpu().numpy(), flags)
        for t in outs:
            t.fill_(GUARD if t.dtype == torch.uint8 else -1515870811)
    assert call(B_=0) == 0 and call(B_=0, src=None, pk=None, npk=0, m=None) == 0
    c.synchronize()
    assert untouched(outs), "no blocks: nothing is touched"
    c.configure("LDPC_AMD_RX_PKT", 0)
    try:
        assert call() == EUNSUP and untouched(outs), "the call has no composed fallback"
    finally:
        c.configure("LDPC_AMD_RX_PKT", None)
    assert call() == 0 and torch.equal(msg, want.msg)


# ------------------------------------------------------------------------------------------------------ 4. the receiver: fused = composed
def make_source(B, k, S, seed):
    return torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def composed_call(c, rx, *args, **kw):
    c.configure("LDPC_AMD_RX_PKT", 0)
    try:
        return rx.rs_decode_many(*args, **kw), c.fec_rs_receiver_info()
    finally:
        c.configure("LDPC_AMD_RX_PKT", None)


def same(a, b):
    return a[0].tolist() == b[0].tolist() and all(torch.equal(x, y) for x, y in zip(a[1:4], b[1:4])) and a[4:] == b[4:]


@pytest.mark.parametrize("W,A,D", rw.WAD)
@pytest.mark.parametrize("k", [192, 223])
def test_rs_decode_many_fused_equals_composed(contexts, k, W, A, D):
    n, S = 255, rw.S
    c, rs = contexts.get("default", n, k)
    B1, B2 = rw.nblocks_for(D)
    src = make_source(B1 + B2, k, S, seed=k + D)
    parts = rw.pieces(lambda f, cnt, b0: c.fec_rs_encode_packets_device(rs, src[f:f + cnt], D, block0=b0).cpu().numpy(), n, k, D, seed=k + 7 * D)
    for max_blocks in (3, 1 << 10):
        cuts = [ic.small_cuts(pk.shape[0], seed=max_blocks + j) for j, pk in enumerate(parts)]
        closed = 0
        with c.fec_rx_window(n, k, S, W, A, depth=D) as fx, c.fec_rx_window(n, k, S, W, A, depth=D) as cx:
            for pk, cut in zip(parts, cuts):
                d_pk = dev(pk)
                edges = [0] + cut + [pk.shape[0]]
                for s, e in zip(edges[:-1], edges[1:]):
                    pos = s
                    while pos < e:
                        f = fx.rs_decode_many(rs, d_pk[pos:e], max_blocks)
                        f_info = c.fec_rs_receiver_info()
                        g, g_info = composed_call(c, cx, rs, d_pk[pos:e], max_blocks)
                        assert (f_info["path"], g_info["path"]) == ("fused", "composed"), (max_blocks, pos)
                        assert same(f, g) and fx.stats() == cx.stats() and fx.state() == cx.state(), (max_blocks, pos)
                        assert f_info["blocks"] == g_info["blocks"] == len(f[0]) and f_info["scratch_bytes"] <= 256 << 20
                        assert (f_info["scratch_bytes"] > 0) == (len(f[0]) > 0)
                        closed += len(f[0])
                        pos += f[4]
                f, g = fx.rs_decode_flush(rs), cx.rs_decode_flush(rs)
                assert c.fec_rs_receiver_info()["path"] == "composed", "the flush is never fused"
                assert f[0].tolist() == g[0].tolist() and all(torch.equal(x, y) for x, y in zip(f[1:], g[1:]))
        assert closed > 0


@pytest.mark.parametrize("n,k,S", [(255, 128, 64), (255, 223, 256)])
def test_receiver_stays_composed_where_the_row_decoder_does_not_apply_or_does_not_win(contexts, n, k, S):
    """n - k = 127 is too deep for the row decoder; at n - k <= 32 and S a multiple of 256 the composed path streams already and wins."""
    B = 12
    c, rs = contexts.get("default", n, k)
    src = make_source(B, k, S, seed=21)
    pk = c.fec_rs_encode_packets_device(rs, src, 1, block0=0)
    keep = torch.rand(pk.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) > 0.05
    pk = pk[keep].contiguous()
    with c.fec_rx_window(n, k, S, 4, 10) as rx:
        blocks, msg, received, status, used = rx.rs_decode_many(rs, pk, 64)
        assert c.fec_rs_receiver_info()["path"] == "composed" and used == pk.shape[0]
        b2, m2, _, s2 = rx.rs_decode_flush(rs)
    got = {int(b): m for b, m, s in zip(blocks.tolist() + b2.tolist(), torch.cat([msg, m2]), status.tolist() + s2.tolist()) if s == 0}
    assert len(got) == B and all(torch.equal(got[b], src[b]) for b in range(B))


# ------------------------------------------------------------------------------------------------------ 5. one object, mixed calls
def test_fused_calls_push_many_and_the_flush_continue_one_another(contexts):
    n, k, S, (W, A, D) = 255, 192, rw.S, rw.WAD[1]
    c, rs = contexts.get("default", n, k)
    B1, B2 = rw.nblocks_for(D)
    src = make_source(B1 + B2, k, S, seed=31)
    pk = rw.pieces(lambda f, cnt, b0: c.fec_rs_encode_packets_device(rs, src[f:f + cnt], D, block0=b0).cpu().numpy(), n, k, D, seed=32)[0]
    third = pk.shape[0] // 3
    d_pk = dev(pk)
    with api.FecRxWindowHost(n, k, S, W, A, depth=D) as hx, c.fec_rx_window(n, k, S, W, A, depth=D) as rx:
        closed = 0
        for step, (s, e) in enumerate([(0, third), (third, 2 * third), (2 * third, pk.shape[0])]):
            hb, hs, he, hu = hx.push_many(pk[s:e], 64)
            if step == 1:    # a plain push_many between the two fused calls
                b, sy, er, u = rx.push_many(d_pk[s:e], 64)
                assert b.tolist() == hb.tolist() and u == hu and np.array_equal(sy.cpu().numpy(), hs) and np.array_equal(er.cpu().numpy(), he)
            else:            # the C call, with the flags
                msg = torch.full((64, k, S), GUARD, dtype=torch.uint8, device="cuda")
                er = torch.full((64, n), 7, dtype=torch.uint8, device="cuda")
                received, status = (torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(2))
                blocks = np.zeros(64, dtype=np.int32)
                used = C.c_int64(0)
                nb = c._L.ldpc_amd_fec_rxw_dev_rs_decode_many(rx._h, rs, d_pk[s:e].data_ptr(), e - s, msg.data_ptr(), received.data_ptr(), status.data_ptr(),
                                                              er.data_ptr(), blocks.ctypes.data, 64, C.byref(used))
                assert c.fec_rs_receiver_info()["path"] == "fused"
                assert nb == len(hb) and used.value == hu and blocks[:nb].tolist() == hb.tolist()
                assert np.array_equal(er[:nb].cpu().numpy(), he) and bool((er[nb:] == 7).all()) and bool((msg[nb:] == GUARD).all())
                if nb:
                    ref = c.rs_decode_frames(rs, hs, he)
                    assert np.array_equal(msg[:nb].cpu().numpy(), ref.msg) and np.array_equal(received[:nb].cpu().numpy(), ref.received)
                    assert np.array_equal(status[:nb].cpu().numpy(), ref.status)
            closed += len(hb)
            assert rx.stats() == hx.stats() and rx.state() == hx.state(), step
        assert closed > 0
        fb, fs, fe = hx.flush()
        gb, gm, gr, gs = rx.rs_decode_flush(rs)
        ref = c.rs_decode_frames(rs, fs, fe)
        assert c.fec_rs_receiver_info()["path"] == "composed"
        assert gb.tolist() == fb.tolist() and np.array_equal(gm.cpu().numpy(), ref.msg) and np.array_equal(gs.cpu().numpy(), ref.status)
        assert rx.stats() == hx.stats() and rx.state() == hx.state()
