"""GPU tests of the link emulator (include/ldpc_erasure_amd_link.h, csrc/link_dev.hip): plan, apply and apply_ragged against the numpy
model tools/link_model.py byte for byte over the plan grid and the payload shapes, whole runs sender -> link -> receiver against a host
api.FecRx fed the MODEL's arriving packets, and the refusals.  Every buffer of the byte-for-byte tests lies between 4 KiB sentinel
bands; outputs are pre-filled with a poison byte."""
import ctypes as C

import numpy as np
import pytest

import link_cases as cases
import wire_ragged_cases as wcases
from code_helpers import random_code
from ldpc_erasure_codes_amd import api, codes, synth
from link_cases import lm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_word_symbols import Arena  # noqa: E402  (4 KiB sentinel bands around every buffer)

EINVAL, EUNSUP = -1, -5
POISON = 0xEE
NAMES = ("out", "sweeps", "residual", "status", "erased_out", "residual_src")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def poisoned(arn, shape, dtype=torch.uint8):
    t = arn.new(shape, dtype)
    t.view(-1).view(torch.uint8).fill_(POISON)
    return t


def is_poison(t):
    return bool((t.contiguous().view(-1).view(torch.uint8) == POISON).all())


def ptr(t):
    return t if t is None or isinstance(t, int) else t.data_ptr()


def link_params(pr):
    return api.LinkParams(pr.seed, pr.first, pr.window, pr.flags, pr.dup, pr.bad_sym, pr.foreign)


def plan_raw(ctx, pr, P, lost, src, fate, cap, count):
    return ctx._L.ldpc_amd_fec_link_plan_dev(ctx._h, C.byref(link_params(pr)), P, ptr(lost), ptr(src), ptr(fate), cap, ptr(count))


def apply_raw(ctx, pk, P, S, src, fate, count, cap, out, flow_of=None, flow_of_out=None):
    return ctx._L.ldpc_amd_fec_link_apply_dev(ctx._h, ptr(pk), P, S, ptr(src), ptr(fate), ptr(count), cap, ptr(out), ptr(flow_of), ptr(flow_of_out))


def ragged_raw(ctx, data, nbytes, off, P, src, fate, count, cap, out, bytes_cap, off_out, total):
    return ctx._L.ldpc_amd_fec_link_apply_ragged_dev(ctx._h, ptr(data), nbytes, ptr(off), P, ptr(src), ptr(fate), ptr(count), cap, ptr(out), bytes_cap,
                                                     ptr(off_out), ptr(total))


def err(ctx):
    return ctx._L.ldpc_amd_last_error(ctx._h)


def u16(t):
    return t.cpu().numpy().view(np.uint16)


def device_lost(ctx, arn, kind, P, first):
    """The loss input of a variant made by the library's own generators on the device, as the header says a caller makes it (n = 1,
    frame0 = first, nframes = P); checked against the numpy generator."""
    want = cases.lost_host(kind, P, first)
    if want is None or P == 0:
        return None, want
    d = poisoned(arn, (P,))
    if kind == "uniform":
        ctx.synth_erasures_uniform(cases.LOSS_SEED, first, P, 1, 0.10, d)
    elif kind == "bursty":
        ctx.synth_erasures_bursty(cases.LOSS_SEED, first, P, 1, *cases.GE, d)
    else:
        d.fill_(1)
    assert np.array_equal(d.cpu().numpy(), want)
    return d, want


# ------------------------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("P,W", cases.GRID)
def test_plan_is_the_models_bytes(ctx, P, W):
    for vi, v in enumerate(cases.VARIANTS):
        pr = cases.params_of(v, W, seed=1000 * P + W + vi)
        arn = Arena()
        d_lost, lost = device_lost(ctx, arn, v[0], P, v[2])
        cap = 2 * P + (3 if vi & 1 else 0)
        src, fate, count = poisoned(arn, (max(cap, 1),), torch.int32), poisoned(arn, (max(cap, 1),), torch.int16), poisoned(arn, (1,), torch.int64)
        assert plan_raw(ctx, pr, P, d_lost, src, fate, cap, count) == 0, err(ctx)
        arn.check()
        w_src, w_fate = lm.plan(pr, P, lost)
        Q = w_src.shape[0]
        tag = (P, W, v)
        assert int(count[0]) == Q, tag
        assert np.array_equal(src.cpu().numpy()[:Q], w_src), tag
        assert np.array_equal(u16(fate)[:Q], w_fate), tag
        assert is_poison(src[Q:]) and is_poison(fate[Q:]), tag               # nothing at or beyond Q is written
        if d_lost is not None:
            assert np.array_equal(d_lost.cpu().numpy(), lost)
        assert ctx.fec_link_info()["plan_packets"] == P
        if vi == 5:                                                          # the same bytes on every run
            src2, fate2, count2 = poisoned(arn, (max(cap, 1),), torch.int32), poisoned(arn, (max(cap, 1),), torch.int16), poisoned(arn, (1,), torch.int64)
            assert plan_raw(ctx, pr, P, d_lost, src2, fate2, cap, count2) == 0
            arn.check()
            assert torch.equal(src2, src) and torch.equal(fate2, fate) and torch.equal(count2, count)


def test_plan_through_the_binding_continues_one_stream(ctx):
    """FecLink advances first by P per call: two calls make the draws of one (the fates per entry), no packet crosses the boundary."""
    P1, P2, first = 700, 500, (1 << 32) - 300
    kw = dict(window=50, dup=0.3, bad_sym=0.1, foreign=0.2, dup_flip=True)
    link = ctx.fec_link(9, first=first, **kw)
    pr = lm.Params(seed=9, first=first, window=50, flags=lm.DUP_FLIP, dup=0.3, bad_sym=0.1, foreign=0.2)
    got = []
    for P in (P1, P2):
        assert link.first == pr.first
        src, fate, count = link.plan(P)
        assert src.shape == (2 * P,) and src.dtype == torch.int32 and fate.dtype == torch.int16 and count.dtype == torch.int64
        Q = int(count[0])
        w_src, w_fate = lm.plan(pr, P)
        assert Q == w_src.shape[0] and np.array_equal(src[:Q].cpu().numpy(), w_src) and np.array_equal(u16(fate[:Q]), w_fate)
        got.append((w_src, w_fate))
        pr = pr._replace(first=pr.first + P)
    assert link.first == first + P1 + P2
    one = lm.draws(pr._replace(first=first), P1 + P2)
    for (s, f), base in zip(got, (0, P1)):
        assert np.array_equal(f, one.fate[s + base, f & lm.COPY])            # every arriving entry has the fate of the single call's draw
    info = ctx.fec_link_info()
    assert info["plan_packets"] == P2 and info["scratch_bytes"] >= 8 * (-(-P1 // cases.TILE) + 1)


# ------------------------------------------------------------------------------------------------------------------ apply
def callers_plan(rng, P, W=40):
    """The model's plan of a busy link, with a few entries a caller planted: sources -1 and P."""
    pr = lm.Params(seed=int(rng.integers(1 << 30)), first=5, window=W, flags=lm.DUP_FLIP, dup=0.3, bad_sym=0.1, foreign=0.2)
    lost = (rng.random(P) < 0.1).astype(np.uint8)
    src, fate = lm.plan(pr, P, lost)
    src, fate = src.copy(), fate.copy()
    at = rng.choice(src.shape[0], size=4, replace=False)
    src[at[:2]], src[at[2:]] = -1, P
    fate[at[0]] = lm.COPY | lm.FLIPPED                                       # (a fate the slot of zeros ignores)
    return src, fate, at


@pytest.mark.parametrize("S", [8, 12, 16, 24, 1024, 1460, 1528])
def test_apply_is_the_models_gather(ctx, S):
    rng = np.random.default_rng(S)
    P, plen = 300, 8 + S
    pk = cases.random_packets(rng, P, S)
    flow = rng.integers(0, 5, size=P).astype(np.int32)
    src, fate, planted = callers_plan(rng, P)
    Q, cap = src.shape[0], 2 * P
    w_out, w_fo = lm.apply(pk, src, fate, flow)
    assert np.array_equal(w_out[planted[1]], lm.badsym_slot(plen)) and (w_fo[planted] == -1).all()
    assert ((fate & lm.BADSYM) != 0).any() and ((fate & lm.FOREIGN) != 0).any() and ((fate & lm.FLIPPED) != 0).any() and (np.diff(src) < 0).any()
    for shift in (0, 4):                                                     # packets_out 16-byte aligned, and 4-byte aligned only
        arn = Arena()
        d_pk, d_flow = arn.new(pk.shape, src=pk), arn.new((P,), torch.int32, src=flow)
        d_src, d_fate = poisoned(arn, (cap,), torch.int32), poisoned(arn, (cap,), torch.int16)
        d_src[:Q], d_fate[:Q] = torch.from_numpy(src).cuda(), torch.from_numpy(fate.view(np.int16)).cuda()
        d_count = arn.new((1,), torch.int64, src=np.array([Q], dtype=np.int64))
        base = poisoned(arn, (shift + cap * plen,))
        out = base[shift:].view(cap, plen)
        assert out.data_ptr() % 16 == shift
        fo = poisoned(arn, (cap,), torch.int32)
        assert apply_raw(ctx, d_pk, P, S, d_src, d_fate, d_count, cap, out, d_flow, fo) == 0, err(ctx)
        out2 = poisoned(arn, (cap, plen))
        assert apply_raw(ctx, d_pk, P, S, d_src, d_fate, d_count, cap, out2) == 0, err(ctx)        # without flows: the same packets
        arn.check()
        assert np.array_equal(out[:Q].cpu().numpy(), w_out), (S, shift)
        assert np.array_equal(fo[:Q].cpu().numpy(), w_fo), (S, shift)
        assert torch.equal(out2[:Q], out[:Q])
        assert is_poison(out[Q:]) and is_poison(fo[Q:]) and is_poison(out2[Q:]) and is_poison(base[:shift])
        assert np.array_equal(d_pk.cpu().numpy(), pk)
    assert ctx.fec_link_info()["apply_packets"] == P


def test_send_through_the_binding(ctx):
    rng = np.random.default_rng(21)
    P, S = 1000, 48
    pk = cases.random_packets(rng, P, S)
    flow = (np.arange(P) % 3).astype(np.int32)
    lost = synth.erasures_uniform(5, 0, P, 1, 0.1).reshape(P)
    link = ctx.fec_link(4, window=64, dup=0.1, bad_sym=0.05, foreign=0.05, dup_flip=True)
    out, fo, src, fate = link.send(torch.from_numpy(pk).cuda(), torch.from_numpy(lost).cuda(), torch.from_numpy(flow).cuda())
    pr = lm.Params(seed=4, first=0, window=64, flags=lm.DUP_FLIP, dup=0.1, bad_sym=0.05, foreign=0.05)
    w_src, w_fate = lm.plan(pr, P, lost)
    w_out, w_fo = lm.apply(pk, w_src, w_fate, flow)
    assert np.array_equal(src.cpu().numpy(), w_src) and np.array_equal(u16(fate), w_fate)
    assert np.array_equal(out.cpu().numpy(), w_out) and np.array_equal(fo.cpu().numpy(), w_fo)
    assert link.first == P
    # a pristine link: the packets unchanged, in order
    out, fo, src, fate = ctx.fec_link(1).send(torch.from_numpy(pk).cuda())
    assert fo is None and np.array_equal(src.cpu().numpy(), np.arange(P)) and not bool(fate.any()) and np.array_equal(out.cpu().numpy(), pk)
    # nothing to send
    out, fo, src, fate = link.send(torch.zeros((0, 8 + S), dtype=torch.uint8, device="cuda"))
    assert out.shape == (0, 8 + S) and src.shape == (0,) and link.first == P


# ----------------------------------------------------------------------------------------------------------- apply, ragged
def trimmed_wire(ctx, rng, F, S):
    """A wire from fec_trim_packets (host bytes and offsets) with one backwards pair and one datagram of 7 bytes planted."""
    pk, _ = wcases.host_packets(rng, F, 10, 7, S, short=2)
    w = ctx.fec_trim_packets(torch.from_numpy(pk).cuda(), 7)
    off = w.offset.cpu().numpy().copy()
    data = w.bytes[:int(off[-1])].cpu().numpy()
    P = off.shape[0] - 1
    a, b = P // 3, 2 * P // 3
    off[a + 1] = off[a] - 5              # datagram a runs backwards; datagram a + 1 starts 5 bytes early
    off[b + 1] = off[b] + 7              # datagram b has 7 bytes; datagram b + 1 takes the rest of it
    return data, off, (a, b)


@pytest.mark.parametrize("S", [8, 48, 1460])
def test_apply_ragged_is_the_models_bytes(ctx, S):
    rng = np.random.default_rng(100 + S)
    data, off, (a, b) = trimmed_wire(ctx, rng, 30, S)
    P, nbytes = off.shape[0] - 1, data.shape[0]
    src, fate, planted = callers_plan(rng, P, W=20)
    free = [q for q in range(src.shape[0]) if q not in planted][:2]
    src[free] = (a, b)                                                       # the two bad datagrams arrive, whatever the loss took
    Q, cap = src.shape[0], 2 * P
    w_by, w_off = lm.apply_ragged(data, off, src, fate)
    ln = np.diff(w_off)
    assert (ln[(src == a) | (src == b)] == 0).all() and (ln[planted] == 0).all() and (ln > 0).sum() > P // 2
    total = int(w_off[-1])
    phases = set()
    for start_in, start_out in ((1, 1), (3, 0), (0, 3), (2, 2)):            # `bytes` and `bytes_out` at odd addresses
        arn = Arena()
        base = arn.new((start_in + nbytes,))
        base[start_in:] = torch.from_numpy(data).cuda()
        d_data = base[start_in:]
        d_off = arn.new((P + 1,), torch.int64, src=off)
        d_src, d_fate = poisoned(arn, (cap,), torch.int32), poisoned(arn, (cap,), torch.int16)
        d_src[:Q], d_fate[:Q] = torch.from_numpy(src).cuda(), torch.from_numpy(fate.view(np.int16)).cuda()
        d_count = arn.new((1,), torch.int64, src=np.array([Q], dtype=np.int64))
        obase = poisoned(arn, (start_out + 2 * nbytes,))
        out = obase[start_out:]
        assert d_data.data_ptr() % 4 == start_in and out.data_ptr() % 4 == start_out
        off_out, tot = poisoned(arn, (cap + 1,), torch.int64), poisoned(arn, (1,), torch.int64)
        assert ragged_raw(ctx, d_data, nbytes, d_off, P, d_src, d_fate, d_count, cap, out, 2 * nbytes, off_out, tot) == 0, err(ctx)
        arn.check()
        tag = (S, start_in, start_out)
        assert np.array_equal(off_out[:Q + 1].cpu().numpy(), w_off), tag
        assert int(tot[0]) == total == int(off_out[Q]), tag
        assert np.array_equal(out[:total].cpu().numpy(), w_by), tag
        assert is_poison(out[total:]) and is_poison(off_out[Q + 1:]) and is_poison(obase[:start_out]), tag
        assert np.array_equal(d_data.cpu().numpy(), data)
        phases |= {(int((d_data.data_ptr() + s) % 4), int((out.data_ptr() + o) % 4)) for s, o, n in
                   zip(off[np.clip(src, 0, P - 1)], w_off[:-1], ln) if n}
        # without total_out: the same
        off2 = poisoned(arn, (cap + 1,), torch.int64)
        out2 = poisoned(arn, (2 * nbytes,))
        assert ragged_raw(ctx, d_data, nbytes, d_off, P, d_src, d_fate, d_count, cap, out2, 2 * nbytes, off2, None) == 0, err(ctx)
        arn.check()
        assert torch.equal(off2[:Q + 1], off_out[:Q + 1]) and np.array_equal(out2[:total].cpu().numpy(), w_by)
    if S != 8:
        assert len(phases) == 16, "every source phase against every destination phase"
    assert ctx.fec_link_info()["apply_ragged_packets"] == P


def test_apply_ragged_never_writes_beyond_bytes_cap(ctx):
    """A caller's own plan that names a packet more than twice asks for more than bytes_cap: the datagrams that would end beyond it
    are not written, the sums still count them."""
    S, P = 1460, 2
    plen = 8 + S
    rng = np.random.default_rng(3)
    data = cases.random_packets(rng, P, S).reshape(-1)
    off = np.arange(P + 1, dtype=np.int64) * plen
    src = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    fate = np.zeros(6, dtype=np.uint16)
    arn = Arena()
    d_data, d_off = arn.new(data.shape, src=data), arn.new((P + 1,), torch.int64, src=off)
    d_src, d_fate = arn.new((6,), torch.int32, src=src), arn.new((6,), torch.int16, src=fate.view(np.int16))
    d_count = arn.new((1,), torch.int64, src=np.array([6], dtype=np.int64))
    out, off_out, tot = poisoned(arn, (2 * P * plen,)), poisoned(arn, (7,), torch.int64), poisoned(arn, (1,), torch.int64)
    assert ragged_raw(ctx, d_data, P * plen, d_off, P, d_src, d_fate, d_count, 6, out, 2 * P * plen, off_out, tot) == 0, err(ctx)
    arn.check()
    assert off_out.tolist() == [q * plen for q in range(7)] and int(tot[0]) == 6 * plen > out.shape[0]
    w_by, _ = lm.apply_ragged(data, off, src[:4], fate[:4])
    assert np.array_equal(out.cpu().numpy(), w_by)


def test_send_wire_through_the_binding(ctx):
    rng = np.random.default_rng(31)
    S = 64
    pk, _ = wcases.host_packets(rng, 40, 10, 7, S, short=3)
    w = ctx.fec_trim_packets(torch.from_numpy(pk).cuda(), 7)
    P = pk.shape[0]
    lost = synth.erasures_uniform(6, 0, P, 1, 0.1).reshape(P)
    link = ctx.fec_link(8, window=33, dup=0.1, bad_sym=0.05, foreign=0.05, dup_flip=True)
    total = int(w.offset[-1])
    got, src, fate = link.send_wire(api.Wire(w.bytes[:total], w.offset), torch.from_numpy(lost).cuda())
    pr = lm.Params(seed=8, first=0, window=33, flags=lm.DUP_FLIP, dup=0.1, bad_sym=0.05, foreign=0.05)
    w_src, w_fate = lm.plan(pr, P, lost)
    w_by, w_off = lm.apply_ragged(w.bytes[:total].cpu().numpy(), w.offset.cpu().numpy(), w_src, w_fate)
    assert isinstance(got, api.Wire) and np.array_equal(src.cpu().numpy(), w_src) and np.array_equal(u16(fate), w_fate)
    assert np.array_equal(got.offset.cpu().numpy(), w_off) and np.array_equal(got.bytes.cpu().numpy(), w_by)
    # landed, the trimmed wire's datagrams are the fixed-stride link's packets
    landed, st = ctx.fec_land_packets(got.bytes, got.offset, S)
    # (but for the flipped copies: the fixed-stride link flips the zeros behind a short datagram too, land fills in zeros)
    w_out, _ = lm.apply(pk, w_src, w_fate)
    plain = (w_fate & lm.FLIPPED) == 0
    assert not bool(st.any()) and np.array_equal(landed.cpu().numpy()[plain], w_out[plain]) and not plain.all()
    # an empty wire
    got, src, fate = link.send_wire(api.Wire(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")))
    assert got.bytes.shape == (0,) and got.offset.tolist() == [0] and src.shape == (0,)


# ------------------------------------------------------------------------------------------------------------ end to end
def to_host(fr, S):
    r = [x.cpu().numpy() for x in fr]
    r[0] = r[0].reshape(r[0].shape[0], -1, S)
    return r


def reference_frames(ctx, h, sym, er, S):
    """The closed blocks of the host receiver decoded by the same context."""
    fr = ctx.decode_frames(h, torch.from_numpy(sym).cuda(), torch.from_numpy(er).cuda())
    ctx.synchronize()
    return to_host(fr, S)


def same_frames(got, want, tag):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (tag, name)


def device_loss(ctx, seed, P, loss):
    lost = torch.empty(P, dtype=torch.uint8, device="cuda")
    return ctx.synth_erasures_uniform(seed, 0, P, 1, loss, lost)


def test_end_to_end_fixed_stride(ctx):
    e = cases.E2E_FIXED
    code = codes.load_builtin(e["code"])
    n, k, S, F = code.n, code.k, e["S"], e["F"]
    assert (n, k) == (2040, 1530)
    h = ctx.load_builtin_code(e["code"], codes.DEFAULT_COEF_SEED[e["code"]])
    source = torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    pk = ctx.fec_encode_packets_device(h, source)
    link = ctx.fec_link(e["seed"], **cases.E2E_LINK)
    arrived, _, src, fate = link.send(pk, device_loss(ctx, e["loss_seed"], F * n, e["loss"]))
    with ctx.fec_rx_device(n, k, S) as rx:
        blocks, fr, used = rx.decode_many(h, arrived, F + 2)
        got = to_host(fr, S)
        last = rx.decode_flush(h)
        assert last is not None and rx.decode_flush(h) is None
        dropped = rx.dropped
    got = [np.concatenate([a, b]) for a, b in zip(got, to_host(last[1], S))]
    # the reference: the MODEL's arriving packets through the host receiver, decoded by the same context
    m_out, _, m_src, m_fate, _ = cases.e2e_model(pk.cpu().numpy(), cases.e2e_params(e["seed"]), e["loss_seed"], e["loss"])
    h_blocks, h_sym, h_er, h_dropped, flushed = cases.host_receiver(m_out, n, k, S, F + 2)
    assert flushed == 1 and used == arrived.shape[0] == m_out.shape[0]
    assert np.array_equal(np.append(blocks, last[0]), h_blocks) and dropped == h_dropped
    same_frames(got, reference_frames(ctx, h, h_sym, h_er, S), "fixed stride")
    assert np.array_equal(src.cpu().numpy(), m_src) and np.array_equal(u16(fate), m_fate) and np.array_equal(arrived.cpu().numpy(), m_out)


def test_end_to_end_multi_flow(ctx):
    e = cases.E2E_FLOWS
    code = random_code()
    n, k, S, nf, per = code.n, code.k, e["S"], e["nflows"], e["per"]
    h = ctx.register_code(code)
    source = torch.randint(0, 256, (nf * per, k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    pk, flow_of, _ = ctx.fec_tx_flows(h, S, nf, block0=list(e["block0"])).send(source, np.arange(nf + 1) * per, api.TX_ROUND_ROBIN)
    P = pk.shape[0]
    kw = dict(cases.E2E_LINK, window=e["window"])
    arrived, fo, _, _ = ctx.fec_link(e["seed"], **kw).send(pk, device_loss(ctx, e["loss_seed"], P, e["loss"]), flow_of)
    m_out, m_fo, _, _, _ = cases.e2e_model(pk.cpu().numpy(), cases.e2e_params(e["seed"], window=e["window"]), e["loss_seed"], e["loss"],
                                           flow_of.cpu().numpy())
    assert np.array_equal(arrived.cpu().numpy(), m_out) and np.array_equal(fo.cpu().numpy(), m_fo)
    with ctx.fec_rx_flows(nf, n, k, S) as rx:
        closes, blocks, fr, consumed, offered = rx.decode_mixed(h, arrived, fo, per + 2)
        got = to_host(fr, S)
        at = np.concatenate([[0], np.cumsum(closes)])
        for f in range(nf):
            h_blocks, h_sym, h_er, h_dropped, flushed = cases.host_receiver(m_out[m_fo == f], n, k, S, per + 2)
            B = h_blocks.shape[0] - flushed
            assert closes[f] == B and np.array_equal(blocks[at[f]:at[f + 1]], h_blocks[:B]), f
            assert offered[f] == consumed[f] == int((m_fo == f).sum())
            want = reference_frames(ctx, h, h_sym, h_er, S)
            same_frames([g[at[f]:at[f + 1]] for g in got], [w[:B] for w in want], ("flow", f))
            for j in range(flushed):
                last = rx.decode_flush(f, h)
                assert last is not None and last[0] == h_blocks[B + j]
                same_frames(to_host(last[1], S), [w[B + j:B + j + 1] for w in want], ("flow", f, "flush", j))
            assert rx.decode_flush(f, h) is None
            assert rx.dropped[f] == h_dropped


def test_end_to_end_ragged(ctx):
    """Datagrams -> pack + encode + trim -> the link on the trimmed wire -> land -> receiver -> unpack: every datagram that is
    delivered equals what was sent.  (No flip here: a flipped copy that arrives last IS what the receiver keeps.)"""
    code = random_code()
    n, k, S, F, b0 = code.n, code.k, 64, 4, 254
    h = ctx.register_code(code)
    rng = np.random.default_rng(12)
    N = F * k - 9
    ln = np.where(rng.random(N) < 0.25, rng.integers(0, S - 3, size=N), S - 4).astype(np.int64)
    ln[::17] = 12
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    host = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    w = ctx.fec_tx_device(h, S, block0=b0).send_datagrams_trimmed(torch.from_numpy(host).cuda(), off)
    total = int(w.offset[-1])
    link = ctx.fec_link(7, **dict(cases.E2E_LINK, window=40, dup_flip=False))
    got, src, fate = link.send_wire(api.Wire(w.bytes[:total], w.offset), device_loss(ctx, 55, F * n, 0.05))
    assert got.bytes.shape[0] < src.shape[0] * (8 + S) and bool((fate != 0).any())
    landed, st = ctx.fec_land_packets(got.bytes, got.offset, S)
    assert not bool(st.any())
    with ctx.fec_rx_device(n, k, S) as rx:
        blocks, fr, used = rx.decode_many(h, landed, F + 2)
        blocks, frs = blocks.tolist(), [fr]
        while True:
            last = rx.decode_flush(h)
            if last is None:
                break
            blocks.append(last[0])
            frs.append(last[1])
    out = torch.cat([f.out for f in frs]).contiguous().view(-1, n, S)
    era = torch.cat([f.erased_out for f in frs]).contiguous()
    dg = ctx.fec_unpack_datagrams(out, k, era)
    state, o, by = dg.state.cpu().numpy(), dg.offset.cpu().numpy(), dg.bytes.cpu().numpy()
    assert len(blocks) >= F - 1
    delivered = 0
    for j, blk in enumerate(blocks):
        f = (blk - b0) & 0xFF
        assert f < F
        for r in range(k):
            i, row = f * k + r, j * k + r
            if state[row] == api.DGRAM_DELIVERED:
                assert i < N and np.array_equal(by[o[row]:o[row + 1]], host[off[i]:off[i + 1]]), (blk, r)
                delivered += 1
            else:
                assert state[row] != api.DGRAM_MALFORMED
    assert delivered > (F - 1) * k // 2


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_every_output_as_poison(ctx):
    rng = np.random.default_rng(13)
    S, P = 16, 40
    plen, cap = 8 + S, 80
    pk_h = cases.random_packets(rng, P, S)
    pr0 = lm.Params(seed=2, first=0, window=8, flags=0, dup=0.2, bad_sym=0.1, foreign=0.1)
    w_src, w_fate = lm.plan(pr0, P)
    Q = w_src.shape[0]
    arn = Arena()
    d_pk = arn.new(pk_h.shape, src=pk_h)
    d_lost = arn.new((P,))
    d_lost.zero_()
    src, fate, count = poisoned(arn, (cap,), torch.int32), poisoned(arn, (cap,), torch.int16), poisoned(arn, (1,), torch.int64)
    g_src, g_fate = arn.new((cap,), torch.int32), arn.new((cap,), torch.int16)                  # a good plan, for apply
    g_src.zero_()
    g_fate.zero_()
    g_src[:Q], g_fate[:Q] = torch.from_numpy(w_src).cuda(), torch.from_numpy(w_fate.view(np.int16)).cuda()
    g_count = arn.new((1,), torch.int64, src=np.array([Q], dtype=np.int64))
    out, fo = poisoned(arn, (cap, plen)), poisoned(arn, (cap,), torch.int32)
    d_flow = arn.new((P,), torch.int32, src=np.zeros(P, dtype=np.int32))
    d_off = arn.new((P + 1,), torch.int64, src=np.arange(P + 1, dtype=np.int64) * plen)
    by, off_out, tot = poisoned(arn, (2 * P * plen,)), poisoned(arn, (cap + 1,), torch.int64), poisoned(arn, (1,), torch.int64)
    host_src, host_pk = np.zeros(cap, dtype=np.int32), pk_h.copy()

    def plan(pr=pr0, **kw):
        a = dict(P=P, lost=d_lost, src=src, fate=fate, cap=cap, count=count)
        a.update(kw)
        return plan_raw(ctx, pr, a["P"], a["lost"], a["src"], a["fate"], a["cap"], a["count"])

    def apply(**kw):
        a = dict(pk=d_pk, P=P, S=S, src=g_src, fate=g_fate, count=g_count, cap=cap, out=out, flow=d_flow, fo=fo)
        a.update(kw)
        return apply_raw(ctx, a["pk"], a["P"], a["S"], a["src"], a["fate"], a["count"], a["cap"], a["out"], a["flow"], a["fo"])

    def ragged(**kw):
        a = dict(data=d_pk, nbytes=P * plen, off=d_off, P=P, src=g_src, fate=g_fate, count=g_count, cap=cap, out=by, bcap=2 * P * plen, oo=off_out, tot=tot)
        a.update(kw)
        return ragged_raw(ctx, a["data"], a["nbytes"], a["off"], a["P"], a["src"], a["fate"], a["count"], a["cap"], a["out"], a["bcap"], a["oo"], a["tot"])

    assert plan(cap=2 * P - 1) == EINVAL and b"cap" in err(ctx)
    assert plan(pr0._replace(window=-1)) == EINVAL and plan(pr0._replace(window=4097)) == EINVAL and b"window" in err(ctx)
    assert plan(pr0._replace(dup=-0.01)) == EINVAL and plan(pr0._replace(dup=1.01)) == EINVAL and plan(pr0._replace(dup=float("nan"))) == EINVAL
    assert plan(pr0._replace(bad_sym=0.6, foreign=0.5)) == EINVAL and b"bad_sym + foreign" in err(ctx)
    assert plan(pr0._replace(flags=2)) == EINVAL
    assert plan(P=1 << 30, cap=1 << 31) == EINVAL and plan(P=-1) == EINVAL
    assert plan(src=host_src.ctypes.data) == EINVAL and b"device pointers" in err(ctx)            # host memory
    assert plan(count=None) == EINVAL and plan(src=None) == EINVAL and plan(fate=None) == EINVAL
    assert plan(src=src.data_ptr() + 2, cap=cap - 1, P=P - 1) == EINVAL and b"aligned" in err(ctx)
    assert plan(fate=src) == EINVAL and b"overlaps" in err(ctx)                                   # overlapping outputs
    assert plan(count=src.data_ptr() + 8) == EINVAL and plan(lost=fate) == EINVAL

    assert apply(S=6) == EUNSUP and apply(S=10) == EUNSUP and b"multiple of 4" in err(ctx)
    assert apply(P=-1) == EINVAL and apply(cap=-1) == EINVAL and apply(cap=1 << 31) == EINVAL
    assert apply(pk=host_pk.ctypes.data) == EINVAL and apply(src=host_src.ctypes.data) == EINVAL  # host memory
    assert apply(out=None) == EINVAL and apply(count=None) == EINVAL and apply(fo=None) == EINVAL and apply(flow=None) == EINVAL
    assert apply(out=out.data_ptr() + 2, cap=cap - 1) == EINVAL
    assert apply(out=d_pk, cap=P) == EINVAL and b"overlaps" in err(ctx)                           # packets_out over the packets
    assert apply(fo=out) == EINVAL and apply(out=g_src.data_ptr() & ~3, cap=1) == EINVAL

    assert ragged(bcap=2 * P * plen - 1) == EINVAL and b"bytes_cap" in err(ctx)
    assert ragged(P=-1) == EINVAL and ragged(nbytes=-1) == EINVAL and ragged(cap=1 << 31) == EINVAL
    assert ragged(data=None) == EINVAL and ragged(data=host_pk.ctypes.data) == EINVAL and ragged(off=None) == EINVAL
    assert ragged(oo=off_out.data_ptr() + 4) == EINVAL and ragged(out=d_pk) == EINVAL and ragged(oo=by) == EINVAL and ragged(tot=off_out) == EINVAL
    with pytest.raises(api.LdpcAmdError, match="window"):
        ctx.fec_link(1, window=5000).plan(10)
    arn.check()
    for t in (src, fate, count, out, fo, by, off_out, tot):
        assert is_poison(t)
    assert np.array_equal(d_pk.cpu().numpy(), pk_h)
    # the context is still usable
    assert plan() == 0 and apply() == 0 and ragged() == 0
    arn.check()
    assert int(count[0]) == Q and np.array_equal(src[:Q].cpu().numpy(), w_src)
    w_out, _ = lm.apply(pk_h, w_src, w_fate)
    assert np.array_equal(out[:Q].cpu().numpy(), w_out)
    assert int(tot[0]) == Q * plen and np.array_equal(by[:Q * plen].cpu().numpy(), w_out.reshape(-1))
