"""GPU tests of the device-resident FEC wire path (include/ldpc_erasure_amd_wire_dev.h): the device packetiser and
reassembler against their host counterparts (csrc/wire.cpp), byte for byte, on streams built on the device -- loss,
re-ordering, duplicates with different payloads, symbol numbers >= n, foreign block numbers, more than 256 blocks --
pushed in calls of uneven sizes with small max_blocks; then encode -> packetise -> channel -> reassemble -> decode
entirely on the device against the same pipeline through the host wire layer."""
import ctypes as C

import numpy as np
import pytest

from ldpc_erasure_codes_amd import api, codes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def channel(pk, n, seed, loss=(0.0, 0.05, 0.1, 0.15), window=120, dup=0.02, dup_flip=True, bad_sym=0.005, foreign=0.005):
    """A lossy, re-ordering, duplicating channel on the device (torch indexing).  Per frame a loss rate from `loss`; every
    packet moves up to `window` places; a fraction `dup` of the kept packets is sent again a little later (with a flipped
    payload if dup_flip: the receiver keeps the last copy); a fraction gets a symbol number >= n, another a random block.
    The defaults keep every block of an n = 300 stream above k + 0.2 (n-k) packets: below that the draft's rule stalls."""
    g = _gen(seed)
    dev = pk.device
    P = pk.shape[0]
    rates = torch.tensor(loss, device=dev)
    frame = torch.arange(P, device=dev) // n
    rate = rates[torch.randint(0, len(loss), (int(frame[-1]) + 1,), device=dev, generator=g)][frame]
    kept = pk[torch.rand(P, device=dev, generator=g) >= rate]
    K = kept.shape[0]
    di = torch.randint(0, K, (max(1, int(K * dup)),), device=dev, generator=g)
    d = kept[di].clone()
    if dup_flip:
        d[:, 8:] ^= 0x5A
    pos = torch.cat([torch.arange(K, device=dev, dtype=torch.float64),
                     di.double() + torch.randint(1, 64, (di.shape[0],), device=dev, generator=g).double()])
    pos = pos + torch.rand(pos.shape[0], device=dev, generator=g, dtype=torch.float64) * window
    out = torch.cat([kept, d])[torch.argsort(pos)].contiguous()
    m = torch.rand(out.shape[0], device=dev, generator=g) < bad_sym
    out[m, 1] = 0xFF                                     # symbol number >= 0xff00 >= n
    m = torch.rand(out.shape[0], device=dev, generator=g) < foreign
    out[m, 2] = torch.randint(0, 256, (int(m.sum()),), device=dev, generator=g, dtype=torch.uint8)
    return out


def run_both(ctx, pk_dev, n, k, S, seed, max_blocks=(1, 2, 3, 5), sizes=(1, 17, 300, 1111, 4000)):
    """The same stream through api.FecRx and FecRxDevice in the same calls; everything they return must be identical.
    Returns the closed blocks in order: (block number, erased flags) of each."""
    rng = np.random.default_rng(seed)
    pk_host = pk_dev.cpu().numpy()
    hrx, drx = api.FecRx(n, k, S), ctx.fec_rx_device(n, k, S)
    closed = []
    pos, P = 0, pk_host.shape[0]
    calls = 0
    while pos < P:
        c, mb = int(rng.choice(sizes)), int(rng.choice(max_blocks))
        hb, hs, he, hu = hrx.push_many(pk_host[pos:pos + c], mb)
        db, ds, de, du = drx.push_many(pk_dev[pos:pos + c], mb)
        assert du == hu and np.array_equal(db, hb), (pos, c, mb)
        assert np.array_equal(ds.cpu().numpy(), hs) and np.array_equal(de.cpu().numpy(), he), (pos, c, mb)
        assert drx.dropped == hrx.dropped
        closed += [(int(b), e) for b, e in zip(hb, he)]
        pos += hu
        calls += 1
    while True:
        h, d = hrx.flush(), drx.flush()
        assert (h is None) == (d is None)
        if h is None:
            break
        assert h[0] == d[0] and np.array_equal(d[1].cpu().numpy(), h[1]) and np.array_equal(d[2].cpu().numpy(), h[2])
        closed.append((h[0], h[2]))
    assert drx.dropped == hrx.dropped
    hrx.close()
    drx.close()
    return closed, calls


# ------------------------------------------------------------------------------------------ packetiser
@pytest.mark.parametrize("n", [300, 2040])
@pytest.mark.parametrize("S", [1, 24, 16, 1024])
def test_packetize_device_matches_host(ctx, n, S):
    F = 8                                                    # blocks 250..257: the 8-bit field wraps
    frames = torch.randint(0, 256, (F, n, S), dtype=torch.uint8, device="cuda", generator=_gen(S * 7 + n))
    pk = ctx.fec_packetize_device(frames, 1, 250)
    ctx.synchronize()
    assert np.array_equal(pk.cpu().numpy(), api.fec_packetize(frames.cpu().numpy(), 1, 250))


def test_packetize_device_unaligned_buffers(ctx):
    n, S, F = 300, 16, 3
    buf = torch.randint(0, 256, (F * n * S + 1,), dtype=torch.uint8, device="cuda", generator=_gen(5))
    frames = buf[1:].view(F, n, S)                           # 1 byte off 16-byte alignment: the byte-wise kernel
    out = torch.zeros(F * n * (8 + S) + 4, dtype=torch.uint8, device="cuda")
    pk = ctx.fec_packetize_device(frames, 7, 3, out=out[4:].view(F * n, 8 + S))
    ctx.synchronize()
    assert np.array_equal(pk.cpu().numpy(), api.fec_packetize(frames.cpu().numpy(), 7, 3))


# ------------------------------------------------------------------------------------------ receiver parity
@pytest.mark.parametrize("S", [16, 24, 1])
def test_rx_device_matches_host_receiver(ctx, S):
    n, k, F = 300, 200, 300                                  # 300 blocks from block 40 on: block numbers wrap
    frames = torch.randint(0, 256, (F, n, S), dtype=torch.uint8, device="cuda", generator=_gen(100 + S))
    pk = channel(ctx.fec_packetize_device(frames, 1, 40), n, seed=200 + S)
    closed, calls = run_both(ctx, pk, n, k, S, seed=S)
    assert calls > 50 and len(closed) > 256                 # past block 255
    assert any(e.any() for _, e in closed)                  # blocks closed with erasures (the 0.8 / 0.2 clauses)


def test_rx_device_matches_host_wide_reorder_large_calls(ctx):
    """Re-order windows of several hundred packets, calls that close many blocks at once, and carried blocks that close in
    the middle of a call."""
    n, k, S, F = 1000, 700, 32, 300
    frames = torch.randint(0, 256, (F, n, S), dtype=torch.uint8, device="cuda", generator=_gen(9))
    pk = channel(ctx.fec_packetize_device(frames, 1, 0), n, seed=10, loss=(0.0, 0.1, 0.2), window=700, dup=0.05)
    closed, _ = run_both(ctx, pk, n, k, S, seed=11, max_blocks=(1, 7, 64), sizes=(5000, 20000, 64, 65))
    assert len(closed) > 256


def test_rx_device_start_rules(ctx):
    """The scripted stream of tests/test_wire.py::test_decode_start_rules: each clause of :139 on its own, a stale block,
    a symbol number beyond n -- one packet per call and the whole stream in one call."""
    n, k, S = 300, 200, 16
    hdr = []
    hdr += [(7, j) for j in range(n)]
    hdr += [(8, j) for j in range(281)] + [(9, j) for j in range(10)] + [(5, 0)] + [(9, 10)]
    hdr += [(9, j) for j in range(11, 221)] + [(10, j) for j in range(101)] + [(10, 400)]
    pk = np.zeros((len(hdr), 8 + S), dtype=np.uint8)
    for i, (b, j) in enumerate(hdr):
        pk[i, :8] = np.frombuffer(api.fec_header_pack(1, b, j).to_bytes(8, "little"), dtype=np.uint8)
        pk[i, 8:] = i & 0xFF
    pk_dev = torch.from_numpy(pk).cuda()
    for per_call in (1, len(hdr)):
        rx = ctx.fec_rx_device(n, k, S)
        got = []
        pos = 0
        while pos < len(hdr):
            b, sym, er, used = rx.push_many(pk_dev[pos:pos + per_call], 8)
            got += [(int(x), int(e.sum())) for x, e in zip(b, er.cpu().numpy())]
            pos += used
        assert got == [(7, 0), (8, n - 281), (9, n - 221)]
        assert rx.dropped == 2
        blk, _, er = rx.flush()
        assert blk == 10 and int((er.cpu().numpy() == 0).sum()) == 101
        assert rx.flush() is None
        rx.close()
    closed, _ = run_both(ctx, pk_dev, n, k, S, seed=3)
    assert [b for b, _ in closed] == [7, 8, 9, 10]


# ------------------------------------------------------------------------------------------ end to end
def _pipeline(ctx, h, n, k, S, F, seed, max_blocks):
    src = torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=_gen(seed))
    cw = ctx.encode(h, src)
    pk = channel(ctx.fec_packetize_device(cw, 1, 0), n, seed=seed + 1, loss=(0.1,), window=300, dup=0.01, dup_flip=False,
                 bad_sym=0.0, foreign=0.0)
    ctx.synchronize()
    pk_host = pk.cpu().numpy()
    drx, hrx = ctx.fec_rx_device(n, k, S), api.FecRx(n, k, S)
    dev_res, host_res, blocks = [], [], []
    pos = 0
    while pos < pk.shape[0]:
        db, ds, de, du = drx.push_many(pk[pos:], max_blocks)
        hb, hs, he, hu = hrx.push_many(pk_host[pos:], max_blocks)
        assert du == hu and np.array_equal(db, hb)
        pos += du
        if len(db):
            out, sw, _, st = ctx.decode(h, ds, de)            # all on the device
            dev_res.append((out.cpu().numpy(), sw.cpu().numpy(), st.cpu().numpy()))
            host_res.append(ctx.decode(h, hs, he))
            blocks += list(db)
    for rx_, dev in ((drx, True), (hrx, False)):
        while True:
            r = rx_.flush()
            if r is None:
                break
            if dev:
                out, sw, _, st = ctx.decode(h, r[1][None].contiguous(), r[2][None].contiguous())
                dev_res.append((out.cpu().numpy(), sw.cpu().numpy(), st.cpu().numpy()))
                blocks.append(r[0])
            else:
                host_res.append(ctx.decode(h, r[1][None], r[2][None]))
    drx.close()
    hrx.close()
    assert len(dev_res) == len(host_res)
    src_h = src.cpu().numpy()
    i, good = 0, 0
    for (o, sw, st), (ho, hsw, _, hst) in zip(dev_res, host_res):
        assert np.array_equal(o, ho) and np.array_equal(sw, hsw) and np.array_equal(st, hst)
        for f in range(o.shape[0]):
            assert blocks[i] == i & 0xFF                     # blocks close in order, one per frame
            if st[f] in (api.ST_MP_DONE, api.ST_ML_SOLVED):
                assert np.array_equal(o[f, :k], src_h[i]), f"block {i}: decodable but not the transmitted source"
                good += 1
            i += 1
    assert i == F and good >= F // 2


def test_end_to_end_device_cfg2_s1024(ctx):
    h = ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])    # cfg 2's (2040,1530) code
    _pipeline(ctx, h, 2040, 1530, 1024, 260, seed=21, max_blocks=64)


def test_end_to_end_device_4080_s16(ctx):
    h = ctx.load_builtin_code(3, codes.DEFAULT_COEF_SEED[3])
    _pipeline(ctx, h, 4080, 3060, 16, 300, seed=31, max_blocks=40)


# ------------------------------------------------------------------------------------------ argument errors
def test_wire_dev_argument_errors(ctx):
    L = api.load_library()
    n, k, S = 300, 200, 16
    frames_h = np.zeros((1, n, S), dtype=np.uint8)
    pk_h = np.zeros((n, 8 + S), dtype=np.uint8)
    frames_d = torch.zeros((1, n, S), dtype=torch.uint8, device="cuda")
    pk_d = torch.zeros((n, 8 + S), dtype=torch.uint8, device="cuda")
    assert L.ldpc_amd_fec_packetize_dev(ctx._h, frames_h.ctypes.data, 1, n, S, 1, 0, pk_d.data_ptr()) == -1
    assert b"device pointers" in L.ldpc_amd_last_error(ctx._h)
    assert L.ldpc_amd_fec_packetize_dev(ctx._h, frames_d.data_ptr(), 1, n, S, 1, 0, pk_h.ctypes.data) == -1
    assert L.ldpc_amd_fec_packetize_dev(ctx._h, frames_d.data_ptr(), 1, 70000, S, 1, 0, pk_d.data_ptr()) == -1
    pinned = torch.zeros((n, 8 + S), dtype=torch.uint8).pin_memory()
    assert L.ldpc_amd_fec_packetize_dev(ctx._h, frames_d.data_ptr(), 1, n, S, 1, 0, pinned.data_ptr()) == -1
    for bad in ((70000, 200, S), (n, n, S), (n, 0, S), (n, 400, S), (n, k, 0)):
        with pytest.raises(api.LdpcAmdError):
            ctx.fec_rx_device(*bad)
    rx = ctx.fec_rx_device(n, k, S)
    with pytest.raises(api.LdpcAmdError):
        rx.push_many(pk_d, 0)                                 # max_blocks < 1
    sym = torch.empty((2, n, S), dtype=torch.uint8, device="cuda")
    er = torch.empty((2, n), dtype=torch.uint8, device="cuda")
    used = C.c_int64(-1)
    sym_h = np.zeros((2, n, S), dtype=np.uint8)
    assert L.ldpc_amd_fec_rx_dev_push_many(rx._h, pk_h.ctypes.data, n, sym.data_ptr(), er.data_ptr(), None, 2, C.byref(used)) == -1
    assert b"device pointers" in L.ldpc_amd_last_error(ctx._h)
    assert L.ldpc_amd_fec_rx_dev_push_many(rx._h, pk_d.data_ptr(), n, sym_h.ctypes.data, er.data_ptr(), None, 2, C.byref(used)) == -1
    assert L.ldpc_amd_fec_rx_dev_push_many(rx._h, pk_d.data_ptr(), 1 << 31, sym.data_ptr(), er.data_ptr(), None, 2, C.byref(used)) == -1
    # nothing was consumed by the refused calls; an empty call is a no-op
    b, _, _, u = rx.push_many(pk_d[:0], 2)
    assert len(b) == 0 and u == 0 and rx.dropped == 0 and rx.flush() is None
    assert L.ldpc_amd_fec_rx_dev_dropped(None) == -1
    rx.close()
