"""GPU tests of word-sized symbols (include/ldpc_erasure_amd_words.h): with symbol unit 4 every payload entry point takes any S that
is a multiple of 4 from 16 bytes up.

Expected values come from the CPU oracle (oracle/liboracle.so takes any S), never from the code under test.  Second, independent
check: the zero-pad identity -- the same input zero-padded to the next multiple of 16 and run on a unit-16 context returns the
same first S bytes of every row and identical sweeps / residual / status / erased_out / residual_src, because the computation is
columnwise over GF(256).  Every device input and output lies in the middle of a larger tensor filled with a sentinel byte, 4 KiB
on each side, and the sentinels must be intact afterwards: an off-by-one row piece is a failed assertion, not an access outside
the allocation.

Shapes (the smallest at which each mechanism can go wrong): S = 20 (16-byte pieces, two of them overlapping by 12, rows 4-byte
aligned), 24 (rows 8-byte aligned), 36 (first S whose piece is wider than 16), 132 and 260 (one full piece of 128 / 256 plus a
4-byte remainder), 1460 (the reference's 367-word packet, OpenCL/device/ldpc_erasure_encoder_VITA_in_UDP_out.cl:141-162)."""
import ctypes as C

import numpy as np
import pytest

from ldpc_erasure_codes_amd import api, codes, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL, EUNSUP = -1, -5
SIZES = (20, 24, 36, 132, 260, 1460)
PERS = (0.10, 0.21, 0.235, 0.27)     # 10 %: message passing completes; the others send frames through the ML stage
PER_FRAMES = 6                       # F = 24
GUARD, SENT = 4096, 0xC3
NAMES = ("out", "sweeps", "residual", "status", "erased_out", "residual_src")
REFUSAL = "S must be 1 or a multiple of 4 that is at least 16 (got %d)"


# ------------------------------------------------------------------------------------------------ contexts and guard bands
@pytest.fixture(scope="module")
def ctx4():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    c.set_symbol_unit(4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx16():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


class Arena:
    """Device tensors in the middle of larger, sentinel-filled ones."""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype=torch.uint8, src=None):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        big = torch.full((GUARD + ((nbytes + 15) & ~15) + GUARD,), SENT, dtype=torch.uint8, device="cuda")
        t = big[GUARD:GUARD + nbytes].view(dtype).view(tuple(shape))
        if src is not None:
            t.copy_(torch.from_numpy(np.array(src)) if isinstance(src, np.ndarray) else src)
        self.bufs.append((big, nbytes))
        return t

    def check(self):
        torch.cuda.synchronize()
        for i, (big, nbytes) in enumerate(self.bufs):
            assert bool((big[:GUARD] == SENT).all()), f"buffer {i}: bytes in front of it were written"
            assert bool((big[GUARD + nbytes:] == SENT).all()), f"buffer {i}: bytes behind it were written"


def pad16(a):
    """Zero-pads the last axis to the next multiple of 16."""
    S = a.shape[-1]
    out = np.zeros(a.shape[:-1] + ((S + 15) & ~15,), dtype=a.dtype)
    out[..., :S] = a
    return out


# ------------------------------------------------------------------------------------------------ the oracle's side, once per shape
_CODES, _CASES = {}, {}


def get_code(which):
    if which not in _CODES:
        from oracle import oracle_py
        code = codes.load_builtin(which)
        _CODES[which] = (code, oracle_py.OracleCode(code))
    return _CODES[which]


def handle(ctx, which):
    key = (id(ctx), which)
    if key not in _CODES:
        _CODES[key] = ctx.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which])
    return _CODES[key]


def oracle_frames(oc, code, sym, er, it, do_ml):
    """DecodedFrames (numpy) from the oracle alone.  The mask of a frame left open (status 2 / 3) is the oracle's out_erased of
    the sweeps (do_ml = 0); status, sweeps and residual depend on the pattern only."""
    F, n, S = sym.shape
    out = np.zeros_like(sym)
    mask = np.zeros((F, n), dtype=np.uint8)
    _, sw, res, st = oc.decode_batch_s1(np.zeros((F, n), dtype=np.uint8), er, itenum=it, do_ml=do_ml)
    for f in range(F):
        out[f], _, it_f, info, _ = oc.decode_packets(sym[f], er[f], itenum=it, do_ml=do_ml)
        assert it_f == sw[f] and info[0] == res[f]
        if st[f] in (2, 3):
            mask[f] = oc.decode_packets(np.zeros((n, 1), dtype=np.uint8), er[f], itenum=it, do_ml=0)[1]
    return api.DecodedFrames(out, sw, res, st, mask, mask[:, :code.k].sum(1).astype(np.int32))


def case(which, S, frames=PER_FRAMES):
    """source, oracle codewords, erasure patterns, received symbols and the oracle's frames (do_ml = 1 and 0) -- computed once and
    shared; nobody writes to them."""
    key = (which, S, frames)
    if key not in _CASES:
        code, oc = get_code(which)
        era = np.concatenate([synth.erasures_uniform(5, 0, frames, code.n, p) for p in PERS])
        F = era.shape[0]
        src = synth.source(40 + S, 0, F, code.k, S)
        cw = np.stack([oc.encode(src[f]) for f in range(F)])
        sym = cw.copy()
        sym[era.astype(bool)] = 0xA5                     # the payload of erased symbols is ignored
        want = {ml: oracle_frames(oc, code, sym, era, 10, ml) for ml in (1, 0)}
        # a case cannot pass by never reaching a stage: message passing alone, ML solved, ML rank-deficient; ML skipped
        assert set(want[1].status.tolist()) >= {0, 1, 2} and 3 in want[0].status.tolist()
        for a in (era, src, cw, sym) + tuple(want[1]) + tuple(want[0]):
            a.setflags(write=False)
        _CASES[key] = dict(code=code, era=era, src=src, cw=cw, sym=sym, want=want, F=F)
    return _CASES[key]


def same(got, want, tag):
    host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)  # noqa: E731
    want = api.DecodedFrames(*[host(x) for x in want])
    for name, a, b in zip(NAMES, got, want):
        a = host(a).reshape(b.shape)
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(1))[0]
        assert bad.size == 0, f"{tag}: {name} differs in frames {bad[:8].tolist()} (status {np.asarray(want.status)[bad[:8]].tolist()})"


def frames_device(ctx, h, n, sym_t, era_t, ar, do_ml, inplace=False):
    """ldpc_amd_decode_frames on guarded device buffers (the Python wrapper allocates its own outputs)."""
    F, _, S = sym_t.shape
    out = sym_t if inplace else ar.new((F, n, S))
    sw, res, st, rsrc = (ar.new((F,), torch.int32) for _ in range(4))
    eo = ar.new((F, n))
    flags = api.DEVICE_PTRS | (api.INPLACE if inplace else 0)
    rc = ctx._L.ldpc_amd_decode_frames(ctx._h, h, S, F, sym_t.data_ptr(), era_t.data_ptr(), 10, do_ml, out.data_ptr(), sw.data_ptr(),
                                       res.data_ptr(), st.data_ptr(), eo.data_ptr(), rsrc.data_ptr(), flags)
    assert rc == 0, ctx._L.ldpc_amd_last_error(ctx._h)
    ar.check()
    return api.DecodedFrames(*[x.cpu().numpy() for x in (out, sw, res, st, eo, rsrc)])


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("S", SIZES)
def test_decode_equals_the_oracle_and_the_padded_run(ctx4, ctx16, S):
    c = case(1, S)
    code, era, sym, F = c["code"], c["era"], c["sym"], c["F"]
    h4, h16 = handle(ctx4, 1), handle(ctx16, 1)
    for do_ml in (1, 0):
        want = c["want"][do_ml]
        # host pointers
        same(ctx4.decode(h4, sym, era, do_ml=do_ml) + tuple(want[4:]), want, f"decode numpy do_ml={do_ml}")
        same(ctx4.decode_frames(h4, sym, era, do_ml=do_ml), want, f"decode_frames numpy do_ml={do_ml}")
        # device pointers, guarded
        ar = Arena()
        dsym, dera = ar.new(sym.shape, src=sym), ar.new(era.shape, src=era)
        o = ctx4.decode(h4, dsym, dera, do_ml=do_ml, out=ar.new(sym.shape), sweeps=ar.new((F,), torch.int32),
                        residual=ar.new((F,), torch.int32), status=ar.new((F,), torch.int32))
        ar.check()
        same(tuple(x.cpu().numpy() for x in o) + tuple(want[4:]), want, f"decode torch do_ml={do_ml}")
        assert np.array_equal(dsym.cpu().numpy(), sym), "an out-of-place decode wrote to its input"
        same(frames_device(ctx4, h4, code.n, dsym, dera, ar, do_ml), want, f"decode_frames torch do_ml={do_ml}")
        same(frames_device(ctx4, h4, code.n, dsym, dera, ar, do_ml, inplace=True), want, f"decode_frames in place do_ml={do_ml}")
        # the zero-pad identity on a unit-16 context
        psym = pad16(sym)
        p = ctx16.decode_frames(h16, psym, era, do_ml=do_ml)
        same((p.out[:, :, :S],) + tuple(p[1:]), want, f"padded numpy do_ml={do_ml}")
        assert not p.out[:, :, S:].any()
        pi = ctx16.decode_frames(h16, torch.from_numpy(psym).cuda(), torch.from_numpy(np.array(era)).cuda(), do_ml=do_ml, inplace=True)
        ctx16.synchronize()
        same((pi.out.cpu().numpy()[:, :, :S],) + tuple(x.cpu().numpy() for x in pi[1:]), want, f"padded in place do_ml={do_ml}")
    assert ctx4.knobs() == ""


def test_decode_1460_runs_tier_two(ctx4):
    """At S = 1460 the plan has two tiers and the case holds frames with more steps than tier 1 takes: tier 2 runs in the test
    above (the bytes of those frames are compared there); here the plan itself."""
    c = case(1, 1460)
    want = c["want"][1]
    h4 = handle(ctx4, 1)
    o = ctx4.decode(h4, c["sym"], c["era"])
    plan = ctx4.last_plan()
    steps = c["era"].sum(1).astype(np.int64) - want.residual            # symbols the sweeps solve = steps of the frame's schedule
    print("tier-1 cap", plan["tier1_cap"], "two tiers", plan["two_tiers"], "piece", plan["packet_bytes_per_workgroup"], "max steps", int(steps.max()))
    assert plan["two_tiers"] == 1 and plan["packet_bytes_per_workgroup"] == 256
    assert int(steps.max()) > plan["tier1_cap"] and int(steps.min()) <= plan["tier1_cap"]
    assert "ldpc_scatter_big_kernel" in ctx4.profile_kernel_names()["apply_tier2"]
    assert np.array_equal(o[0], want.out)


def test_decode_4080_3060_at_132(ctx4, ctx16):
    c = case(3, 132, frames=2)
    code, era, sym, F = c["code"], c["era"], c["sym"], c["F"]
    h4, h16 = handle(ctx4, 3), handle(ctx16, 3)
    want = c["want"][1]
    same(ctx4.decode_frames(h4, sym, era), want, "numpy")
    ar = Arena()
    dsym, dera = ar.new(sym.shape, src=sym), ar.new(era.shape, src=era)
    same(frames_device(ctx4, h4, code.n, dsym, dera, ar, 1), want, "torch")
    same(frames_device(ctx4, h4, code.n, dsym, dera, ar, 1, inplace=True), want, "in place")
    p = ctx16.decode_frames(h16, pad16(sym), era)
    same((p.out[:, :, :132],) + tuple(p[1:]), want, "padded")
    cw = ctx4.encode(h4, c["src"])
    assert np.array_equal(cw, c["cw"])


@pytest.mark.parametrize("knob,value", [("APPLY", "gather"), ("SCATTER_NT", "0"), ("SCATTER_NT", "1"), ("SCATTER_DYN", "0"), ("ML_PI", "0")])
def test_knobs_do_not_change_the_bytes(ctx4, knob, value):
    c = case(1, 260)
    h4 = handle(ctx4, 1)
    ar = Arena()
    dsym, dera = ar.new(c["sym"].shape, src=c["sym"]), ar.new(c["era"].shape, src=c["era"])
    ref = frames_device(ctx4, h4, c["code"].n, dsym, dera, ar, 1)
    same(ref, c["want"][1], "no knob")
    ctx4.configure(knob, value)
    try:
        got = frames_device(ctx4, h4, c["code"].n, dsym, dera, ar, 1)
        if knob == "APPLY":
            assert ctx4.profile_kernel_names()["apply"] == "ldpc_apply_words_kernel"
    finally:
        ctx4.configure(knob, None)
    same(got, ref, f"{knob}={value}")
    assert ctx4.knobs() == ""


# ------------------------------------------------------------------------------------------------ encode, fused sender
@pytest.mark.parametrize("S", SIZES)
def test_encode_and_fused_sender(ctx4, ctx16, S):
    c = case(1, S)
    code, src, cw, F = c["code"], c["src"], c["cw"], c["F"]
    h4, h16 = handle(ctx4, 1), handle(ctx16, 1)
    assert np.array_equal(ctx4.encode(h4, src), cw), "encode numpy"
    ar = Arena()
    dsrc = ar.new(src.shape, src=src)
    out = ctx4.encode(h4, dsrc, out=ar.new(cw.shape))
    ar.check()
    assert np.array_equal(out.cpu().numpy(), cw), "encode torch"
    pk = ctx4.fec_encode_packets_device(h4, dsrc, 1, 3, out=ar.new((F * code.n, 8 + S)))
    ar.check()
    assert np.array_equal(pk.cpu().numpy(), api.fec_packetize(cw, 1, 3)), "fused sender"
    info = ctx4.fec_sender_info()
    print("S", S, "sender", info["path"], ctx4.profile_kernel_names()["apply"])
    if S in (20, 1460):
        assert info["path"] == "fused"
    ctx4.configure("ENC_PKT", "0")
    try:
        pk2 = ctx4.fec_encode_packets_device(h4, dsrc, 1, 3, out=ar.new((F * code.n, 8 + S)))
        ar.check()
        assert ctx4.fec_sender_info()["path"] == "composed"
    finally:
        ctx4.configure("ENC_PKT", None)
    assert torch.equal(pk, pk2)
    assert np.array_equal(ctx16.encode(h16, pad16(src))[:, :, :S], cw), "padded"


# ------------------------------------------------------------------------------------------------ receiver
def lossy_reordered(pk, n, seed, loss=(0.05, 0.10, 0.15), window=150):
    """Per block a loss rate from `loss`; every surviving packet moves up to `window` places."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    P = pk.shape[0]
    blk = torch.arange(P, device="cuda") // n
    rate = torch.tensor(loss, device="cuda")[torch.randint(0, len(loss), (P // n,), device="cuda", generator=g)][blk]
    kept = pk[torch.rand(P, device="cuda", generator=g) >= rate]
    pos = torch.arange(kept.shape[0], device="cuda", dtype=torch.float64)
    pos = pos + torch.rand(kept.shape[0], device="cuda", generator=g, dtype=torch.float64) * window
    return kept[torch.argsort(pos)].contiguous()


def host_run(pk_host, n, k, S, sizes, max_blocks):
    """The stream through the host reassembler api.FecRx: per call what it was given and what it returned; then the flushes."""
    hrx = api.FecRx(n, k, S)
    calls, pos, i = [], 0, 0
    while pos < pk_host.shape[0]:
        cnt = sizes[i % len(sizes)]
        i += 1
        hb, hs, he, hu = hrx.push_many(pk_host[pos:pos + cnt], max_blocks)
        assert hu > 0
        calls.append(dict(pos=pos, c=cnt, blocks=hb.copy(), sym=hs, er=he, used=hu, dropped=hrx.dropped))
        pos += hu
    flushes = []
    while True:
        r = hrx.flush()
        if r is None:
            break
        flushes.append(r)
    hrx.close()
    return calls, flushes


def rx_many(ctx, rx, h, pk, mb, ar):
    """ldpc_amd_fec_rx_dev_decode_many on guarded output buffers."""
    n, S = rx.n, rx.S
    out = ar.new((mb, n, S))
    sw, res, st, rsrc = (ar.new((mb,), torch.int32) for _ in range(4))
    eo = ar.new((mb, n))
    blocks = np.zeros(mb, dtype=np.int32)
    used = C.c_int64(0)
    nb = ctx._L.ldpc_amd_fec_rx_dev_decode_many(rx._h, h, pk.data_ptr(), pk.shape[0], 10, 1, out.data_ptr(), sw.data_ptr(), res.data_ptr(),
                                                st.data_ptr(), eo.data_ptr(), rsrc.data_ptr(), blocks.ctypes.data, mb, C.byref(used))
    assert nb >= 0, ctx._L.ldpc_amd_last_error(ctx._h)
    ar.check()
    return blocks[:nb], api.DecodedFrames(*[x[:nb].cpu().numpy() for x in (out, sw, res, st, eo, rsrc)]), used.value


def rx_flush(ctx, rx, h, ar):
    n, S = rx.n, rx.S
    out = ar.new((1, n, S))
    sw, res, st, rsrc = (ar.new((1,), torch.int32) for _ in range(4))
    eo = ar.new((1, n))
    blk = C.c_int(-1)
    rc = ctx._L.ldpc_amd_fec_rx_dev_decode_flush(rx._h, h, 10, 1, out.data_ptr(), sw.data_ptr(), res.data_ptr(), st.data_ptr(), eo.data_ptr(),
                                                 rsrc.data_ptr(), C.byref(blk))
    assert rc >= 0, ctx._L.ldpc_amd_last_error(ctx._h)
    ar.check()
    return (blk.value, api.DecodedFrames(*[x.cpu().numpy() for x in (out, sw, res, st, eo, rsrc)])) if rc == 1 else None


@pytest.mark.parametrize("rx_pkt", [1, 0])
@pytest.mark.parametrize("S", [20, 1460])
def test_receiver_equals_push_many_plus_decode_frames_and_the_oracle(ctx4, S, rx_pkt):
    code, oc = get_code(1)
    h4 = handle(ctx4, 1)
    n, k, B = code.n, code.k, 7
    src = synth.source(90 + S, 0, B, k, S)
    cw = np.stack([oc.encode(src[f]) for f in range(B)])          # the stream is built from the oracle's codewords
    ar = Arena()
    pk = lossy_reordered(torch.from_numpy(api.fec_packetize(cw, 1, 250)).cuda(), n, seed=7)
    pk = ar.new(pk.shape, src=pk)
    calls, flushes = host_run(pk.cpu().numpy(), n, k, S, sizes=(5000, 3000, 6000), max_blocks=4)
    assert sum(len(c["blocks"]) for c in calls) + len(flushes) >= 6
    ctx4.configure("RX_PKT", str(rx_pkt))
    rx, rx2 = ctx4.fec_rx_device(n, k, S), ctx4.fec_rx_device(n, k, S)
    try:
        closed = 0
        for i, c in enumerate(calls):
            part = pk[c["pos"]:c["pos"] + c["c"]]
            b, fr, used = rx_many(ctx4, rx, h4, part, 4, ar)
            assert used == c["used"] and np.array_equal(b, c["blocks"]) and rx.dropped == c["dropped"], i
            b2, sym2, er2, used2 = rx2.push_many(part, 4)          # the same receiver state, the two calls apart
            assert used2 == used and np.array_equal(b2, b)
            if len(b):
                closed += len(b)
                info = ctx4.fec_receiver_info()
                assert info["path"] == ("fused" if rx_pkt else "composed") and info["blocks"] == len(b)
                same(fr, ctx4.decode_frames(h4, sym2.contiguous(), er2.contiguous()), f"call {i}: push_many + decode_frames")
                ctx4.synchronize()
                same(fr, oracle_frames(oc, code, c["sym"], c["er"], 10, 1), f"call {i}: oracle")
        assert closed >= 1
        for blk, sym, er in flushes:
            r = rx_flush(ctx4, rx, h4, ar)
            assert r is not None and r[0] == blk
            r2 = rx2.flush()
            assert r2 is not None and r2[0] == blk
            same(r[1], ctx4.decode_frames(h4, r2[1][None].contiguous(), r2[2][None].contiguous()), f"flush {blk}: flush + decode_frames")
            ctx4.synchronize()
            same(r[1], oracle_frames(oc, code, sym[None], er[None], 10, 1), f"flush {blk}: oracle")
        assert rx_flush(ctx4, rx, h4, ar) is None
    finally:
        rx.close()                                                 # (a receiver is closed before its context, on every path)
        rx2.close()
        ctx4.configure("RX_PKT", None)
    assert ctx4.knobs() == ""


# ------------------------------------------------------------------------------------------------ Reed-Solomon
_RS = {}


def rs_case(S, B=8, n=255, k=223):
    """Source, oracle codewords, per block the received positions (block 0: the first k of them; block 5 received fewer than k),
    the oracle's decode of every byte column."""
    if S not in _RS:
        from oracle import oracle_py
        rng = np.random.default_rng(200 + S)
        g = oracle_py.rs_generator(n, k)
        src = rng.integers(0, 256, (B, k, S), dtype=np.uint8)
        cw = np.zeros((B, n, S), dtype=np.uint8)
        for b in range(B):
            for s in range(S):
                cw[b, :, s] = oracle_py.rs_encode(g, np.ascontiguousarray(src[b, :, s]))
        era = (rng.random((B, n)) < 0.08).astype(np.uint8)
        era[1] = 0
        era[2, :n - k] = 1
        era[2, n - k:] = 0                                       # exactly k received, every repair symbol needed
        era[5] = 0
        era[5, rng.choice(n, n - k + 3, replace=False)] = 1      # short: k - 3 received
        assert all((1 - era[b]).sum() >= k for b in range(B) if b != 5)
        idx = np.zeros((B, k), dtype=np.uint16)
        msg = np.zeros((B, k, S), dtype=np.uint8)
        for b in range(B):
            if b == 5:
                continue
            idx[b] = np.nonzero(era[b] == 0)[0][:k]
            for s in range(S):
                m, rc = oracle_py.rs_decode(g, idx[b], np.ascontiguousarray(cw[b, idx[b], s]))
                assert rc == 0
                msg[b, :, s] = m
        assert np.array_equal(np.delete(msg, 5, 0), np.delete(src, 5, 0))
        sym = cw.copy()
        sym[era.astype(bool)] = 0x5A
        _RS[S] = dict(src=src, cw=cw, era=era, idx=idx, msg=msg, sym=sym, received=(1 - era).sum(1).astype(np.int32))
    return _RS[S]


@pytest.mark.parametrize("S", [20, 132, 1460])
def test_rs_equals_the_oracle(ctx4, ctx16, S):
    n, k, B = 255, 223, 8
    c = rs_case(S)
    L = ctx4._L
    rs4, rs16 = ctx4.rs_create(n, k), ctx16.rs_create(n, k)
    # encode
    assert np.array_equal(ctx4.rs_encode(rs4, n, k, c["src"]), c["cw"]), "rs_encode numpy"
    ar = Arena()
    dsrc, dcw = ar.new(c["src"].shape, src=c["src"]), ar.new(c["cw"].shape)
    assert L.ldpc_amd_rs_encode_batch(ctx4._h, rs4, S, B, dsrc.data_ptr(), dcw.data_ptr(), api.DEVICE_PTRS) == 0
    ar.check()
    assert np.array_equal(dcw.cpu().numpy(), c["cw"]), "rs_encode torch"
    assert np.array_equal(ctx16.rs_encode(rs16, n, k, pad16(c["src"]))[:, :, :S], c["cw"]), "rs_encode padded"
    # decode from gathered rows (the short block has no k positions: left out)
    keep = [b for b in range(B) if b != 5]
    idx = np.ascontiguousarray(c["idx"][keep])
    val = np.ascontiguousarray(np.stack([c["cw"][b, c["idx"][b]] for b in keep]))
    want = c["msg"][keep]
    assert np.array_equal(ctx4.rs_decode(rs4, idx, val), want), "rs_decode numpy"
    didx = ar.new((len(keep), 2 * k), src=idx.view(np.uint8))       # (the positions are u16: moved as bytes)
    dmsg = ctx4.rs_decode(rs4, didx, ar.new(val.shape, src=val), out=ar.new(want.shape))
    ar.check()
    assert np.array_equal(dmsg.cpu().numpy(), want), "rs_decode torch"
    assert np.array_equal(ctx16.rs_decode(rs16, idx, pad16(val))[:, :, :S], want), "rs_decode padded"
    # decode from erased frames: the short block is RS_ST_SHORT and all zeros
    r = ctx4.rs_decode_frames(rs4, c["sym"], c["era"])
    assert np.array_equal(r.msg, c["msg"]) and not r.msg[5].any(), "rs_decode_frames numpy"
    assert np.array_equal(r.received, c["received"])
    assert r.status.tolist() == [api.RS_ST_SHORT if b == 5 else api.RS_ST_DECODED for b in range(B)]
    dsym, dera = ar.new(c["sym"].shape, src=c["sym"]), ar.new(c["era"].shape, src=c["era"])
    fmsg, frecv, fst = ar.new(c["msg"].shape), ar.new((B,), torch.int32), ar.new((B,), torch.int32)
    assert L.ldpc_amd_rs_decode_frames(ctx4._h, rs4, S, B, dsym.data_ptr(), dera.data_ptr(), fmsg.data_ptr(), frecv.data_ptr(), fst.data_ptr(),
                                       api.DEVICE_PTRS) == 0
    ar.check()
    assert np.array_equal(fmsg.cpu().numpy(), c["msg"]), "rs_decode_frames torch"
    assert np.array_equal(frecv.cpu().numpy(), r.received) and np.array_equal(fst.cpu().numpy(), r.status)
    p = ctx16.rs_decode_frames(rs16, pad16(c["sym"]), c["era"])
    assert np.array_equal(p.msg[:, :, :S], c["msg"]) and np.array_equal(p.received, r.received) and np.array_equal(p.status, r.status)


# ------------------------------------------------------------------------------------------------ the interface
def test_the_switch(ctx16):
    L = api.load_library()
    code, oc = get_code(1)
    with api.Context(0) as ctx:
        h = ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
        assert ctx.symbol_unit() == 16
        assert L.ldpc_amd_set_symbol_unit(ctx._h, 8) == EINVAL and ctx.symbol_unit() == 16
        ctx.set_symbol_unit(4)
        assert L.ldpc_amd_set_symbol_unit(ctx._h, 8) == EINVAL and ctx.symbol_unit() == 4
        with pytest.raises(api.LdpcAmdError):
            ctx.set_symbol_unit(0)
        era = np.zeros((1, code.n), dtype=np.uint8)
        rs = ctx.rs_create(15, 11)
        for S in (18, 12, 4, 8, 30):
            text = (REFUSAL % S).encode()
            sym = np.zeros((1, code.n, S), dtype=np.uint8)
            out = np.zeros_like(sym)
            i32 = np.zeros(3, dtype=np.int32)
            rc = L.ldpc_amd_decode_batch(ctx._h, h, S, 1, sym.ctypes.data, era.ctypes.data, 10, 1, out.ctypes.data, i32[0:].ctypes.data,
                                         i32[1:].ctypes.data, i32[2:].ctypes.data, 0)
            assert rc == EUNSUP and L.ldpc_amd_last_error(ctx._h) == text
            rc = L.ldpc_amd_encode_batch(ctx._h, h, S, 1, sym.ctypes.data, out.ctypes.data, 0)
            assert rc == EUNSUP and L.ldpc_amd_last_error(ctx._h) == text
            rc = L.ldpc_amd_rs_encode_batch(ctx._h, rs, S, 1, sym.ctypes.data, out.ctypes.data, 0)
            assert rc == EUNSUP and L.ldpc_amd_last_error(ctx._h) == text
            rc = L.ldpc_amd_rs_decode_frames(ctx._h, rs, S, 1, sym.ctypes.data, era.ctypes.data, out.ctypes.data, None, None, 0)
            assert rc == EUNSUP and L.ldpc_amd_last_error(ctx._h) == text
            d = torch.zeros(code.n * (8 + S) + 64, dtype=torch.uint8, device="cuda")
            rc = L.ldpc_amd_fec_encode_packets_dev(ctx._h, h, S, 1, d.data_ptr(), 1, 0, d.data_ptr())
            assert rc == EUNSUP and L.ldpc_amd_last_error(ctx._h) == text
            rx = ctx.fec_rx_device(code.n, code.k, S)               # the receiver is created for any S; its decode refuses
            rc = L.ldpc_amd_fec_rx_dev_decode_flush(rx._h, h, 10, 1, d.data_ptr(), None, None, None, None, None, None)
            err = L.ldpc_amd_last_error(ctx._h)
            rx.close()
            assert rc == EUNSUP and err == text
        # the context is usable afterwards, and a multiple of 16 gives the bytes of a unit-16 context
        era = synth.erasures_uniform(5, 0, 4, code.n, 0.12)
        src = synth.source(9, 0, 4, code.k, 1024)
        cw = ctx.encode(h, src)
        h16 = handle(ctx16, 1)
        assert np.array_equal(cw, ctx16.encode(h16, src))
        sym = cw.copy()
        sym[era.astype(bool)] = 0
        a, b = ctx.decode_frames(h, sym, era), ctx16.decode_frames(h16, sym, era)
        same(a, b, "S = 1024, unit 4 against unit 16")
        assert ctx.profile_kernel_names() == ctx16.profile_kernel_names()
        assert ctx.knobs() == "" and "SYMBOL" not in ctx.knobs().upper()
        ctx.set_symbol_unit(16)
        sym24 = np.zeros((1, code.n, 24), dtype=np.uint8)
        with pytest.raises(api.LdpcAmdError, match="multiple of 16"):
            ctx.decode(h, sym24, np.zeros((1, code.n), dtype=np.uint8))
