"""GPU tests of the fused receiver (include/ldpc_erasure_amd_receiver.h): FEC wire packets on the device straight to decoded frames.

The expected values are built WITHOUT the code under test: the host reassembler api.FecRx (csrc/wire.cpp) gives the closed blocks,
their received symbols and flags, the consumed and dropped counts; the CPU oracle (oracle.OracleCode.decode_packets, or
decode_batch_s1 for S = 1) gives out / sweeps / residual / status and the masks.  On top of that: tier 2 and the ML stage behind
the packets-in kernels, which path ran, equality with push_many + decode_frames in any mix of the calls, the bound of the composed
path's scratch, guard bands around every output, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

from code_helpers import random_code  # noqa: F401  (other test modules take it from here)
from ldpc_erasure_codes_amd import api, codes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL, ENOCODE, EUNSUP = -1, -4, -5
MIB = 1 << 20
NAMES = ("out", "sweeps", "residual", "status", "erased_out", "residual_src")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


_CODES = {}


def get_code(ctx, which):
    """(handle, codes.Code) of a built-in code, the random (300,200) code ("rand") or test_gpu_sender's heavy-column code."""
    if which not in _CODES:
        if which == "rand":
            code = random_code()
            _CODES[which] = (ctx.register_code(code), code)
        elif which == "heavy":
            from test_gpu_sender import heavy_code
            code = heavy_code()
            _CODES[which] = (ctx.register_code(code), code)
        else:
            _CODES[which] = (ctx.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which]), codes.load_builtin(which))
    return _CODES[which]


def make_stream(ctx, h, code, S, F, seed, block0=0, **chan):
    """encode -> packetise on the device -> test_gpu_wire_device's channel."""
    from test_gpu_wire_device import channel
    src = torch.randint(0, 256, (F, code.k, S), dtype=torch.uint8, device="cuda", generator=_gen(seed))
    cw = ctx.encode(h, src[:, :, 0].contiguous() if S == 1 else src)
    pk = ctx.fec_packetize_device(cw.view(F, code.n, S), 1, block0)
    return channel(pk, code.n, seed=seed + 1, **chan)


def lossy_stream(ctx, h, code, S, F, seed, loss):
    """The same without re-ordering: every packet is dropped with probability `loss`."""
    src = torch.randint(0, 256, (F, code.k, S), dtype=torch.uint8, device="cuda", generator=_gen(seed))
    cw = ctx.encode(h, src[:, :, 0].contiguous() if S == 1 else src)
    pk = ctx.fec_packetize_device(cw.view(F, code.n, S), 1, 0)
    return pk[torch.rand(pk.shape[0], device="cuda", generator=_gen(seed + 1)) >= loss].contiguous()


# ---------------------------------------------------------------------------------------------- the reference side
def host_calls(pk_host, n, k, S, seed, sizes, max_blocks):
    """The stream through api.FecRx in calls of mixed sizes: per call what it was given and what it returned; then the flushes."""
    rng = np.random.default_rng(seed)
    hrx = api.FecRx(n, k, S)
    calls, pos, P = [], 0, pk_host.shape[0]
    while pos < P:
        c, mb = int(rng.choice(sizes)), int(rng.choice(max_blocks))
        hb, hs, he, hu = hrx.push_many(pk_host[pos:pos + c], mb)
        assert hu > 0
        calls.append(dict(pos=pos, c=c, mb=mb, blocks=hb.copy(), sym=hs, er=he, used=hu, dropped=hrx.dropped))
        pos += hu
    flushes = []
    while True:
        r = hrx.flush()
        if r is None:
            break
        flushes.append(r)
    hrx.close()
    return calls, flushes


def carried_blocks(pk_host, calls, n):
    """Closed blocks that hold more received symbols than the packets of their own call brought: the rest was received by an
    earlier call and waited in a staging plane."""
    sym = pk_host[:, 0].astype(np.int64) | (pk_host[:, 1].astype(np.int64) << 8)
    blk = pk_host[:, 2].astype(np.int64)
    count = 0
    for c in calls:
        s, b = sym[c["pos"]:c["pos"] + c["used"]], blk[c["pos"]:c["pos"] + c["used"]]
        for j, bn in enumerate(c["blocks"]):
            here = np.unique(s[(b == bn) & (s < n)]).size
            count += int(n - int(c["er"][j].sum()) > here)
    return count


def oracle_frames(oc, code, sym, er, it, do_ml):
    """DecodedFrames (numpy) of the blocks sym [B][n][S], er [B][n] from the CPU oracle alone.  The mask is the oracle's out_erased
    of the sweeps (do_ml = 0) for the frames left open (status 2 / 3), zero for the others; status, sweeps and residual depend on the
    pattern only and come from the oracle's batch entry point."""
    B, n, S = sym.shape
    out = np.zeros_like(sym)
    mask = np.zeros((B, n), dtype=np.uint8)
    _, sw, res, st = oc.decode_batch_s1(np.zeros((B, n), dtype=np.uint8), er, itenum=it, do_ml=do_ml)
    for f in range(B):
        if S == 1:
            out[f, :, 0] = oc.decode_batch_s1(sym[f:f + 1, :, 0], er[f:f + 1], itenum=it, do_ml=do_ml)[0][0]
        else:
            out[f], _, sw[f], info, _ = oc.decode_packets(sym[f], er[f], itenum=it, do_ml=do_ml)
            res[f] = info[0]
        if st[f] in (2, 3):
            mask[f] = oc.decode_packets(np.zeros((n, 1), dtype=np.uint8), er[f], itenum=it, do_ml=0)[1]
    return api.DecodedFrames(out, sw, res, st, mask, mask[:, :code.k].sum(1).astype(np.int32))


def to_host(fr, S):
    r = [x.cpu().numpy() for x in fr]
    r[0] = r[0].reshape(r[0].shape[0], -1, S)
    return api.DecodedFrames(*r)


def same_frames(got, want, tag):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (tag, name)


def run_decode_many(ctx, h, code, S, pk, calls, flushes, oc, it=10, do_ml=1, seen=None):
    """The device receiver over the host run's call boundaries; every call and the flushes against host receiver + oracle.
    Returns the oracle's frames of all blocks, in order.  seen: a dict that receives the launch plan and the kernel names of the
    last decode_many that closed a block (the flushes behind it are single-frame decodes from an array of rows)."""
    rx = ctx.fec_rx_device(code.n, code.k, S)
    wants = []
    for i, c in enumerate(calls):
        b, fr, used = rx.decode_many(h, pk[c["pos"]:c["pos"] + c["c"]], c["mb"], max_sweeps=it, do_ml=do_ml)
        assert used == c["used"] and np.array_equal(b, c["blocks"]) and rx.dropped == c["dropped"], (i, c["pos"], c["c"], c["mb"])
        if len(b):
            want = oracle_frames(oc, code, c["sym"], c["er"], it, do_ml)
            ctx.synchronize()
            same_frames(to_host(fr, S), want, (i, c["pos"], c["c"], c["mb"]))
            wants.append(want)
            if seen is not None:
                seen.update(plan=ctx.last_plan(), names=ctx.profile_kernel_names(), info=ctx.fec_receiver_info())
    for blk, sym, er in flushes:
        r = rx.decode_flush(h, max_sweeps=it, do_ml=do_ml)
        assert r is not None and r[0] == blk
        want = oracle_frames(oc, code, sym[None], er[None], it, do_ml)
        ctx.synchronize()
        same_frames(to_host(r[1], S), want, ("flush", blk))
        wants.append(want)
    assert rx.decode_flush(h) is None
    rx.close()
    return api.DecodedFrames(*[np.concatenate(x) for x in zip(*wants)])


# ---------------------------------------------------------------------------------------------- 1. bytes against host receiver + oracle
# (code, S, F, block0); F = 300 from block 40 wraps the block number
CASES = [(1, 1024, 24, 0), (1, 128, 70, 250), (1, 16, 70, 0), ("rand", 16, 300, 40), ("rand", 128, 300, 40)]


@pytest.mark.parametrize("which,S,F,block0", CASES)
def test_decode_many_equals_host_receiver_and_oracle(ctx, oracle, which, S, F, block0):
    h, code = get_code(ctx, which)
    assert np.bincount(code.cols, minlength=code.n).max() <= 16
    pk = make_stream(ctx, h, code, S, F, seed=300 + S + F, block0=block0)
    pk_host = pk.cpu().numpy()
    sizes = (1, 17, 300, 1111, 4000) if code.n == 300 else (1, 17, 300, 1111, 4000, 9000)
    calls, flushes = host_calls(pk_host, code.n, code.k, S, seed=S + F, sizes=sizes, max_blocks=(1, 2, 3, 64))
    assert sum(len(c["blocks"]) for c in calls) + len(flushes) >= F - 3
    assert carried_blocks(pk_host, calls, code.n) >= 1      # some rows come from the staging planes
    assert any(len(c["blocks"]) == 0 for c in calls)        # calls that close nothing launch no decode
    all_ = run_decode_many(ctx, h, code, S, pk, calls, flushes, oracle.OracleCode(code))
    assert ctx.fec_receiver_info()["path"] == "fused"
    assert all_.erased_out.shape[0] >= F - 3 and (all_.sweeps > 1).any()


# ---------------------------------------------------------------------------------------------- 2. tier 2 and the ML stage
def test_tier2_and_ml_stage_behind_the_packet_kernels(ctx, oracle):
    h, code = get_code(ctx, 1)
    n, k, S, F = code.n, code.k, 1024, 24
    pk = make_stream(ctx, h, code, S, F, seed=77, loss=(0.05, 0.17), bad_sym=0.002, foreign=0.002)
    pk_host = pk.cpu().numpy()
    calls, flushes = host_calls(pk_host, n, k, S, seed=5, sizes=(9000, 30000), max_blocks=(3, 64))
    ers = np.concatenate([c["er"] for c in calls] + [f[2][None] for f in flushes])
    assert ers.shape[0] == F                                 # the host receiver closes every block
    oc = oracle.OracleCode(code)
    seen = {}
    want = run_decode_many(ctx, h, code, S, pk, calls, flushes, oc, it=10, do_ml=1, seen=seen)
    plan, names = seen["plan"], seen["names"]
    lost = ers.sum(1)
    assert plan["two_tiers"] == 1 and (lost > plan["tier1_cap"]).any() and (lost < plan["tier1_cap"]).any()
    assert names["apply"].startswith("ldpc_scatter_pktin_kernel<") and names["apply_tier2"].startswith("ldpc_scatter_pktin_big_kernel<")
    assert seen["info"]["path"] == "fused"
    assert (want.status == 0).all()
    # two sweeps leave the 0.17 frames open: the ML stage takes them (do_ml = 1), or they stay open (do_ml = 0)
    want = run_decode_many(ctx, h, code, S, pk, calls, flushes, oc, it=2, do_ml=1)
    assert (want.status == 1).any()
    want = run_decode_many(ctx, h, code, S, pk, calls, flushes, oc, it=2, do_ml=0)
    open_ = want.status == 3
    assert open_.any() and want.erased_out[open_].any(1).all()
    assert not want.out[want.erased_out.astype(bool)].any()  # rows never solved are zero-filled


# ---------------------------------------------------------------------------------------------- 3. the path is the one promised
def _one_call(c, h, code, S, pk, max_blocks=64, **kw):
    rx = c.fec_rx_device(code.n, code.k, S)
    b, fr, used = rx.decode_many(h, pk, max_blocks, **kw)
    c.synchronize()
    rx.close()
    return b, to_host(fr, S), used


def test_dispatch():
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        assert c.fec_receiver_info() == {"path": "none", "scratch_bytes": 0, "blocks": 0}
        code = codes.load_builtin(1)
        h = c.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
        pk = {S: lossy_stream(c, h, code, S, 6, seed=40 + S, loss=0.08) for S in (1024, 16, 1)}
        for S in (1024, 16):
            b, fused, _ = _one_call(c, h, code, S, pk[S])
            assert len(b) >= 4 and c.fec_receiver_info() == {"path": "fused", "scratch_bytes": 0, "blocks": len(b)}
        _one_call(c, h, code, 1, pk[1])
        assert c.fec_receiver_info()["path"] == "composed"
        from test_gpu_sender import heavy_code
        hv = heavy_code()
        hh = c.register_code(hv)
        pkh = lossy_stream(c, hh, hv, 128, 6, seed=50, loss=0.0)
        keep = torch.ones(pkh.shape[0], dtype=torch.bool, device="cuda")
        keep[torch.arange(6, device="cuda") * hv.n + 5] = False          # one packet lost per block: the close rule needs 44 of 48
        _one_call(c, hh, hv, 128, pkh[keep].contiguous())
        assert c.fec_receiver_info()["path"] == "composed"
        # the knob
        b0, fused, u0 = _one_call(c, h, code, 1024, pk[1024])
        assert c.fec_receiver_info()["path"] == "fused" and c.knobs() == ""
        c.configure("LDPC_AMD_RX_PKT", 0)
        assert "RX_PKT=0" in c.knobs()
        b1, composed, u1 = _one_call(c, h, code, 1024, pk[1024])
        info = c.fec_receiver_info()
        assert info["path"] == "composed" and 0 < info["scratch_bytes"] <= 256 * MIB
        assert u0 == u1 and np.array_equal(b0, b1)
        same_frames(composed, fused, "RX_PKT=0")
        c.configure("LDPC_AMD_RX_PKT", None)
        assert c.knobs() == ""
        _one_call(c, h, code, 1024, pk[1024])
        assert c.fec_receiver_info()["path"] == "fused"
        # a packets view 1 byte off 8-byte alignment
        buf = torch.zeros(pk[1024].numel() + 8, dtype=torch.uint8, device="cuda")
        off = buf[1:1 + pk[1024].numel()].view(pk[1024].shape)
        off.copy_(pk[1024])
        assert off.data_ptr() % 8 == 1
        b2, odd, u2 = _one_call(c, h, code, 1024, off)
        assert c.fec_receiver_info()["path"] == "composed" and u2 == u0 and np.array_equal(b2, b0)
        same_frames(odd, fused, "odd packets pointer")


# ---------------------------------------------------------------------------------------------- 4. same bytes as the two calls
def two_calls(ctx, rx, h, S, pk, mb):
    """push_many + decode_frames: what the library offered before decode_many."""
    b, sym, er, used = rx.push_many(pk, mb)
    fr = None
    if len(b):
        fr = ctx.decode_frames(h, sym[:, :, 0].contiguous() if S == 1 else sym, er)
    return b, fr, used


def run_mix(ctx, h, code, S, pk, bounds, pick):
    """The stream in the calls `bounds` = [(size, max_blocks)], call i made through decode_many if pick(i) else through the two calls."""
    rx = ctx.fec_rx_device(code.n, code.k, S)
    pos, blocks, frames = 0, [], []
    for i, (c, mb) in enumerate(bounds):
        if pos >= pk.shape[0]:
            break
        b, fr, used = rx.decode_many(h, pk[pos:pos + c], mb) if pick(i) else two_calls(ctx, rx, h, S, pk[pos:pos + c], mb)
        pos += used
        if len(b):
            ctx.synchronize()
            blocks += [int(x) for x in b]
            frames.append(to_host(fr, S))
    assert pos == pk.shape[0]
    while True:
        r = rx.decode_flush(h)
        if r is None:
            break
        ctx.synchronize()
        blocks.append(r[0])
        frames.append(to_host(r[1], S))
    dropped = rx.dropped
    rx.close()
    return blocks, api.DecodedFrames(*[np.concatenate(x) for x in zip(*frames)]), dropped


@pytest.mark.parametrize("which,S,F", [(1, 1024, 12), (1, 16, 20), (1, 1, 20), (3, 16, 20), (0, 256, 20)])
def test_any_mix_of_the_calls_gives_the_same_bytes(ctx, which, S, F):
    h, code = get_code(ctx, which)
    pk = make_stream(ctx, h, code, S, F, seed=500 + S, loss=(0.0, 0.05, 0.1))
    rng = np.random.default_rng(S)
    n = code.n
    bounds = [(int(rng.choice((1, 17, n // 3, n, 3 * n + 5))), int(rng.choice((1, 2, 64)))) for _ in range(4000)]
    ref = run_mix(ctx, h, code, S, pk, bounds, lambda i: False)
    assert len(ref[0]) >= F - 2
    for name, pick in (("all", lambda i: True), ("decode_many first", lambda i: i < 12), ("push_many first", lambda i: i >= 12),
                       ("alternating", lambda i: i % 2 == 0)):
        got = run_mix(ctx, h, code, S, pk, bounds, pick)
        assert got[0] == ref[0] and got[2] == ref[2], name
        same_frames(got[1], ref[1], name)


# ---------------------------------------------------------------------------------------------- 5. the composed scratch is bounded
def test_composed_scratch_is_bounded():
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        code = codes.load_builtin(1)
        h = c.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
        n, S, F = code.n, 1024, 300                          # 627 MB of received symbols
        frames = torch.randint(0, 256, (F, n, S), dtype=torch.uint8, device="cuda", generator=_gen(6))
        pk = c.fec_packetize_device(frames, 1, 0)
        del frames
        pk = pk[torch.rand(pk.shape[0], device="cuda", generator=_gen(7)) >= 0.03].contiguous()
        b0, fused, u0 = _one_call(c, h, code, S, pk, max_blocks=300)
        assert c.fec_receiver_info()["path"] == "fused" and len(b0) >= F - 2
        c.configure("LDPC_AMD_RX_PKT", 0)
        b1, composed, u1 = _one_call(c, h, code, S, pk, max_blocks=300)
        info = c.fec_receiver_info()
        assert info["path"] == "composed" and info["blocks"] == len(b0)
        assert 0 < info["scratch_bytes"] <= 256 * MIB
        assert u0 == u1 and np.array_equal(b0, b1)
        same_frames(composed, fused, "300 blocks in one call")


# ---------------------------------------------------------------------------------------------- 6. guard bands
@pytest.mark.parametrize("S,knob", [(1024, None), (16, None), (1024, 0), (1, None)])
def test_guard_bands_and_untouched_slots(ctx, S, knob):
    h, code = get_code(ctx, 1)
    n, k = code.n, code.k
    pk = lossy_stream(ctx, h, code, S, 5, seed=60 + S, loss=0.1)
    before = pk.clone()
    L = ctx._L
    MB, G = 8, 4096                                          # slots offered, guard bytes on both sides
    sizes = dict(out=MB * n * S, sweeps=4 * MB, residual=4 * MB, status=4 * MB, erased_out=MB * n, residual_src=4 * MB)
    bufs = {kk: torch.full((v + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda") for kk, v in sizes.items()}
    ptr = {kk: bufs[kk].data_ptr() + G for kk in bufs}
    ctx.configure("LDPC_AMD_RX_PKT", knob)
    try:
        rx = ctx.fec_rx_device(n, k, S)
        blocks = np.zeros(MB, dtype=np.int32)
        used = C.c_int64(0)
        nb = L.ldpc_amd_fec_rx_dev_decode_many(rx._h, h, pk.data_ptr(), pk.shape[0], 10, 1, ptr["out"], ptr["sweeps"], ptr["residual"],
                                               ptr["status"], ptr["erased_out"], ptr["residual_src"], blocks.ctypes.data, MB, C.byref(used))
        ctx.synchronize()
        rx.close()
    finally:
        ctx.configure("LDPC_AMD_RX_PKT", None)
    assert 3 <= nb < MB and used.value == pk.shape[0]
    assert torch.equal(pk, before)                           # the packet array is only read
    for kk, v in sizes.items():
        per = v // MB
        host = bufs[kk].cpu().numpy()
        assert (host[:G] == 0xA5).all() and (host[G + v:] == 0xA5).all(), kk
        assert (host[G + nb * per:G + v] == 0xA5).all(), f"{kk}: slots at or beyond closes were touched"
    st = bufs["status"][G:G + 4 * nb].view(torch.int32).cpu().numpy()
    assert (st == 0).all()


# ---------------------------------------------------------------------------------------------- 7. argument errors
def test_receiver_argument_errors(ctx, oracle):
    L = ctx._L
    h, code = get_code(ctx, 1)
    hr, rcode = get_code(ctx, "rand")
    n, k, S, F = code.n, code.k, 16, 6
    pk = make_stream(ctx, h, code, S, F, seed=90, loss=(0.05, 0.1))
    pk_host = pk.cpu().numpy()
    cut = pk.shape[0] // 2 + 7
    calls, flushes = host_calls(pk_host, n, k, S, seed=1, sizes=(cut,), max_blocks=(64,))
    oc = oracle.OracleCode(code)
    MB = 64
    out = torch.full((MB, n, S), 0xA5, dtype=torch.uint8, device="cuda")
    i32 = torch.zeros((4, MB), dtype=torch.int32, device="cuda")
    eo = torch.zeros((MB, n), dtype=torch.uint8, device="cuda")
    blocks = np.zeros(MB, dtype=np.int32)
    used = C.c_int64(-1)
    rx = ctx.fec_rx_device(n, k, S)
    # the first half of the stream goes in, then every refused call, then the rest: the results must be the reference's
    c0 = calls[0]
    b, fr, u = rx.decode_many(h, pk[:cut], MB)
    assert u == c0["used"] and np.array_equal(b, c0["blocks"])
    ctx.synchronize()
    same_frames(to_host(fr, S), oracle_frames(oc, code, c0["sym"], c0["er"], 10, 1), "first half")
    rest = pk[c0["used"]:]

    def call(code_h=h, packets=rest.data_ptr(), np_=rest.shape[0], it=10, out_p=out.data_ptr(), mb=MB, rxh=None):
        return L.ldpc_amd_fec_rx_dev_decode_many(rxh or rx._h, code_h, packets, np_, it, 1, out_p, i32[0].data_ptr(), i32[1].data_ptr(),
                                                 i32[2].data_ptr(), eo.data_ptr(), i32[3].data_ptr(), blocks.ctypes.data, mb, C.byref(used))

    def refused(rc, want, text=None):
        assert rc == want
        msg = L.ldpc_amd_last_error(ctx._h)
        assert msg and (text is None or text in msg), msg

    rest_host = np.ascontiguousarray(pk_host[c0["used"]:])
    refused(call(packets=rest_host.ctypes.data), EINVAL, b"device pointer")
    pinned = torch.zeros(rest.shape, dtype=torch.uint8).pin_memory()
    refused(call(packets=pinned.data_ptr()), EINVAL, b"device pointer")
    out_host = np.zeros((MB, n, S), dtype=np.uint8)
    refused(call(out_p=out_host.ctypes.data), EINVAL, b"device pointers")
    refused(call(code_h=hr), EINVAL, b"(300,200)")
    refused(call(code_h=999), ENOCODE, b"unknown code handle")
    refused(call(it=0), EINVAL, b"max_sweeps must be >= 1")
    refused(call(mb=0), EINVAL, b"max_blocks")
    rx24 = ctx.fec_rx_device(n, k, 24)
    pk24 = torch.zeros((50, 8 + 24), dtype=torch.uint8, device="cuda")
    refused(call(packets=pk24.data_ptr(), np_=50, rxh=rx24._h), EUNSUP, b"S must be 1 or a multiple of 16 (got 24)")
    refused(L.ldpc_amd_fec_rx_dev_decode_flush(rx24._h, h, 10, 1, out.data_ptr(), None, None, None, None, None, None), EUNSUP, b"multiple of 16")
    rx24.close()
    refused(L.ldpc_amd_fec_rx_dev_decode_flush(rx._h, h, 0, 1, out.data_ptr(), None, None, None, None, None, None), EINVAL, b"max_sweeps")
    # npackets = 0: returns 0, nothing is touched (not even looked at: null pointers pass)
    assert call(packets=None, np_=0, out_p=None) == 0 and used.value == 0
    ctx.synchronize()
    assert bool((out == 0xA5).all()) and rx.dropped == c0["dropped"]
    # ... and the stream goes on as if nothing had happened
    c1 = calls[1]
    b, fr, u = rx.decode_many(h, rest[:c1["c"]], MB)
    assert u == c1["used"] and np.array_equal(b, c1["blocks"]) and rx.dropped == c1["dropped"]
    ctx.synchronize()
    same_frames(to_host(fr, S), oracle_frames(oc, code, c1["sym"], c1["er"], 10, 1), "second half")
    rx.close()
