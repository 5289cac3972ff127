"""GPU tests of the datagram calls (include/ldpc_erasure_amd_datagrams.h, csrc/datagram_dev.hip): pack and unpack against the numpy
model tools/datagram_frames.py byte for byte, the refusals, and datagrams of mixed lengths through the sender, a lossy channel,
the receiver and unpack, with the CPU oracle stating beforehand what the channel allows to come back."""
import os
import sys

import numpy as np
import pytest

from code_helpers import random_code
from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import datagram_frames as dg  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL, EUNSUP = -1, -5
K = 7
TILE = 256          # rows per tile of the unpack scan (kTile of datagram_dev.hip)
SCAN_ROUND = 1024   # tile sums one round of the scan workgroup's loop takes (kThreads * kScanPer)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def lengths(rng, N, S, p_special=0.5):
    """The edge lengths 0, 1, 2, 3, 4, 5, S - 5, S - 4 (where S admits them) mixed with random ones."""
    pool = [v for v in (0, 1, 2, 3, 4, 5, S - 5, S - 4) if 0 <= v <= S - 4]
    return np.array([int(rng.choice(pool)) if rng.random() < p_special else int(rng.integers(0, S - 3)) for _ in range(N)], dtype=np.int64)


def offsets_of(ln, first=0):
    return np.concatenate([[first], first + np.cumsum(ln)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ pack
@pytest.mark.parametrize("S", [8, 16, 48, 1460])
@pytest.mark.parametrize("N", [1, K - 1, K, K + 1, 5 * K + 3])
def test_pack_is_the_models_bytes_at_every_source_phase(ctx, S, N):
    rng = np.random.default_rng(1000 * S + N)
    ln = lengths(rng, N, S)
    if N == 1:
        ln[0] = S - 5
    off = offsets_of(ln, first=int(rng.integers(0, 8)))
    host = rng.integers(0, 256, size=int(off[-1]) + 8, dtype=np.uint8)
    F = -(-N // K)
    phases = set()
    for start in (0, 1, 2, 3):
        # `data` is a slice that starts `start` bytes into its tensor (torch allocations are at least 256-byte aligned)
        base = torch.zeros(start + host.shape[0], dtype=torch.uint8, device="cuda")
        base[start:] = torch.from_numpy(host).cuda()
        data = base[start:]
        assert data.data_ptr() % 4 == start
        phases |= {int((data.data_ptr() + o) % 4) for o, l in zip(off[:-1], ln) if l}
        out = torch.full((F, K, S), 0xA5, dtype=torch.uint8, device="cuda")
        got = ctx.fec_pack_datagrams(data, off, K, S, out=out)
        assert got is out
        assert np.array_equal(out.cpu().numpy(), dg.pack(host, off, K, S)), (S, N, start)
    assert phases == {0, 1, 2, 3}
    assert ctx.fec_dgram_info()["pack_rows"] == F * K


def test_pack_allocates_its_result_and_takes_fillers_only(ctx):
    S, N = 16, 10
    off = np.full(N + 1, 3, dtype=np.int64)
    data = torch.arange(64, dtype=torch.uint8, device="cuda")
    out = ctx.fec_pack_datagrams(data, off, K, S)
    assert tuple(out.shape) == (2, K, S) and not out.cpu().numpy().any()
    # two calls back to back, the second with other offsets: both right (the staging slots are not reused under a copy in flight)
    rng = np.random.default_rng(3)
    host = rng.integers(0, 256, size=4096, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    offs = [offsets_of(lengths(rng, 40, 48)) for _ in range(5)]
    outs = [ctx.fec_pack_datagrams(dev, o, K, 48) for o in offs]
    for o, t in zip(offs, outs):
        assert np.array_equal(t.cpu().numpy(), dg.pack(host, o, K, 48))
    info = ctx.fec_dgram_info()
    assert info["scratch_bytes"] > 0 and info["staging_bytes"] > 0


def test_pack_zero_datagrams_touches_nothing(ctx):
    L = ctx._L
    off = np.zeros(1, dtype=np.int64)
    assert L.ldpc_amd_fec_dgram_pack_dev(ctx._h, None, off.ctypes.data, 0, K, 16, None) == 0
    assert tuple(ctx.fec_pack_datagrams(torch.zeros(4, dtype=torch.uint8, device="cuda"), off, K, 16).shape) == (0, K, 16)


def test_pack_refusals_leave_the_output_alone(ctx):
    S = 16
    data = torch.arange(200, dtype=torch.uint8, device="cuda")
    out = torch.full((1, K, S), 0xA5, dtype=torch.uint8, device="cuda")   # (every call below has at most K datagrams: one frame)
    L = ctx._L

    def raw(d, off, k=K, s=S, o=out, n=None):
        off = np.ascontiguousarray(off, dtype=np.int64)
        return L.ldpc_amd_fec_dgram_pack_dev(ctx._h, d, off.ctypes.data, off.shape[0] - 1 if n is None else n, k, s, o.data_ptr() if o is not None else None)

    with pytest.raises(api.LdpcAmdError, match="datagram 2 has 13 bytes"):
        ctx.fec_pack_datagrams(data, [0, 5, 10, 10 + S - 3, 30], K, S, out=out)                 # a length of S - 3, at index 2
    with pytest.raises(api.LdpcAmdError, match="non-decreasing"):
        ctx.fec_pack_datagrams(data, [0, 8, 4, 12], K, S, out=out)                              # decreasing offsets
    with pytest.raises(api.LdpcAmdError, match="device pointers"):
        ctx.fec_pack_datagrams(np.arange(200, dtype=np.uint8), [0, 8, 12], K, S, out=out)       # a numpy `data`
    out10 = torch.full((1, K, 10), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(api.LdpcAmdError, match="multiple of 4"):
        ctx.fec_pack_datagrams(data, [0, 4], K, 10, out=out10)                                  # S = 10
    assert raw(data.data_ptr(), [0, 4], s=4) == EUNSUP
    assert raw(data.data_ptr(), [-1, 4]) == EINVAL
    assert raw(data.data_ptr(), [0, 4], k=0) == EINVAL
    assert raw(data.data_ptr(), [0, 4], n=-1) == EINVAL
    assert raw(data.data_ptr(), [0, 4], o=None) == EINVAL
    assert raw(None, [0, 4]) == EINVAL
    assert L.ldpc_amd_fec_dgram_pack_dev(ctx._h, data.data_ptr(), None, 1, K, S, out.data_ptr()) == EINVAL
    assert L.ldpc_amd_fec_dgram_pack_dev(ctx._h, data.data_ptr(), np.array([0, 4], dtype=np.int64).ctypes.data, 1, K, S, out.data_ptr() + 2) == EINVAL   # alignment
    both = torch.full((4 * K * S,), 0xA5, dtype=torch.uint8, device="cuda")
    assert L.ldpc_amd_fec_dgram_pack_dev(ctx._h, both.data_ptr() + K * S - 4, np.array([0, 8], dtype=np.int64).ctypes.data, 1, K, S, both.data_ptr()) == EINVAL   # overlap
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and (out10 == 0xA5).all() and (both == 0xA5).all()
    # the context is still usable
    got = ctx.fec_pack_datagrams(data, [0, 5, 17], K, S, out=out)
    assert np.array_equal(got.cpu().numpy(), dg.pack(np.arange(200, dtype=np.uint8), [0, 5, 17], K, S))


# ---------------------------------------------------------------------------------------------------------------- unpack
def make_frames(rng, B, n, k, S, p_erased=0.2, p_filler=0.1, malformed=4):
    """Frames whose source rows are datagram symbols (all lengths, so every destination phase occurs), repair rows noise, some
    rows erased (and overwritten with noise: their prefix must not be read), some prefixes planted malformed."""
    N = B * k
    ln = rng.integers(0, S - 3, size=N).astype(np.int64)
    ln[rng.random(N) < p_filler] = 0
    off = offsets_of(ln)
    data = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    frames = rng.integers(0, 256, size=(B, n, S), dtype=np.uint8)
    frames[:, :k] = dg.pack(data, off, k, S)
    erased = (rng.random((B, n)) < p_erased).astype(np.uint8)
    frames[erased.astype(bool)] = rng.integers(0, 256, size=(int(erased.sum()), S), dtype=np.uint8)
    bad = []
    for j, r in enumerate(rng.choice(N, size=min(malformed, N), replace=False)):
        v = [S - 3, 0xFFFFFFFF, S, 1 << 31][j % 4]
        frames[r // k, r % k, :4] = np.frombuffer(np.uint32(v).astype("<u4").tobytes(), dtype=np.uint8)
        bad.append(int(r))
    return frames, erased, bad


def unpack_raw(ctx, frames, erased, k, cap=None, slack=64):
    """The C call on tensors of the test's own: bytes_out prefilled with 0xA5 and `slack` bytes longer than cap."""
    B, n, S = frames.shape
    R = B * k
    cap = R * (S - 4) if cap is None else cap
    by = torch.full((max(cap, 0) + slack,), 0xA5, dtype=torch.uint8, device="cuda")
    off = torch.full((R + 1,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((R,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = ctx._L.ldpc_amd_fec_dgram_unpack_dev(ctx._h, frames.data_ptr(), erased.data_ptr() if erased is not None else None, B, n, k, S,
                                              by.data_ptr(), cap, off.data_ptr(), st.data_ptr())
    return rc, by, off, st


def check_unpack(ctx, frames, erased, k):
    d_fr = torch.from_numpy(frames).cuda()
    d_er = torch.from_numpy(erased).cuda() if erased is not None else None
    rc, by, off, st = unpack_raw(ctx, d_fr, d_er, k)
    assert rc == 0, ctx._L.ldpc_amd_last_error(ctx._h)
    w_by, w_off, w_st = dg.unpack(frames, k, erased)
    assert np.array_equal(st.cpu().numpy(), w_st)
    assert np.array_equal(off.cpu().numpy(), w_off)
    by = by.cpu().numpy()
    total = int(w_off[-1])
    assert np.array_equal(by[:total], w_by)
    assert (by[total:] == 0xA5).all()          # nothing at or beyond the total is written
    return w_st


@pytest.mark.parametrize("S", [8, 16, 48, 1460])
@pytest.mark.parametrize("B,k", [(3, 85), (4, 64), (1, 257)])   # B * k one below, at and one above the scan tile
def test_unpack_is_the_models_bytes_around_the_scan_tile(ctx, S, B, k):
    assert B * k - TILE == {85: -1, 64: 0, 257: 1}[k]
    rng = np.random.default_rng(S * 7 + k)
    frames, erased, bad = make_frames(rng, B, k + 5, k, S)
    st = check_unpack(ctx, frames, erased, k)
    assert set(st.tolist()) == {dg.DELIVERED, dg.FILLER, dg.LOST, dg.MALFORMED} or S == 8
    assert ctx.fec_dgram_info()["unpack_rows"] == B * k


@pytest.mark.parametrize("B,k", [(4096, 64), (37500, 7)])   # 1024 tiles: one round of the tile-sum scan exactly; 1026: a second round
def test_unpack_when_the_tile_sum_scan_loops(ctx, B, k):
    tiles = -(-B * k // TILE)
    assert (tiles > SCAN_ROUND) == (k == 7) and tiles >= SCAN_ROUND
    rng = np.random.default_rng(k)
    frames, erased, _ = make_frames(rng, B, k + 1, k, 8, malformed=16)
    check_unpack(ctx, frames, erased, k)


def test_unpack_without_flags_and_through_the_binding(ctx):
    rng = np.random.default_rng(11)
    k, S = 33, 48
    frames, _, bad = make_frames(rng, 9, k + 4, k, S)
    st = check_unpack(ctx, frames, None, k)
    assert dg.LOST not in st.tolist() and (st[bad] == dg.MALFORMED).all()
    frames, erased, _ = make_frames(rng, 9, k + 4, k, S)
    got = ctx.fec_unpack_datagrams(torch.from_numpy(frames).cuda(), k, torch.from_numpy(erased).cuda())
    assert isinstance(got, api.Datagrams) and got.bytes.shape[0] == 9 * k * (S - 4)
    w_by, w_off, w_st = dg.unpack(frames, k, erased)
    assert np.array_equal(got.state.cpu().numpy(), w_st) and np.array_equal(got.offset.cpu().numpy(), w_off)
    assert np.array_equal(got.bytes[:int(w_off[-1])].cpu().numpy(), w_by)


def test_unpack_refusals_touch_nothing(ctx):
    rng = np.random.default_rng(12)
    k, S, B = 20, 16, 3
    frames, erased, _ = make_frames(rng, B, k + 2, k, S)
    d_fr, d_er = torch.from_numpy(frames).cuda(), torch.from_numpy(erased).cuda()
    need = B * k * (S - 4)
    rc, by, off, st = unpack_raw(ctx, d_fr, d_er, k, cap=need - 1)          # a cap one too small
    assert rc == EINVAL and b"cap" in ctx._L.ldpc_amd_last_error(ctx._h)
    torch.cuda.synchronize()
    assert (by == 0xA5).all() and (off == -1).all() and (st == 0xA5).all()
    L, h = ctx._L, ctx._h
    args = lambda **kw: [kw.get(a, d) for a, d in (("fr", d_fr.data_ptr()), ("er", d_er.data_ptr()), ("B", B), ("n", k + 2), ("k", k), ("S", S),   # noqa: E731
                                                   ("by", by.data_ptr()), ("cap", need), ("off", off.data_ptr()), ("st", st.data_ptr()))]
    assert L.ldpc_amd_fec_dgram_unpack_dev(h, *args(S=10)) == EUNSUP
    assert L.ldpc_amd_fec_dgram_unpack_dev(h, *args(S=4)) == EUNSUP
    assert L.ldpc_amd_fec_dgram_unpack_dev(h, *args(k=0)) == EINVAL
    assert L.ldpc_amd_fec_dgram_unpack_dev(h, *args(n=k - 1)) == EINVAL
    assert L.ldpc_amd_fec_dgram_unpack_dev(h, *args(B=-1)) == EINVAL
    assert L.ldpc_amd_fec_dgram_unpack_dev(h, *args(fr=frames.ctypes.data)) == EINVAL          # host memory
    assert L.ldpc_amd_fec_dgram_unpack_dev(h, *args(st=None)) == EINVAL
    assert L.ldpc_amd_fec_dgram_unpack_dev(h, *args(off=off.data_ptr() + 4)) == EINVAL         # alignment
    assert L.ldpc_amd_fec_dgram_unpack_dev(h, *args(by=d_fr.data_ptr())) == EINVAL             # an output over an input
    assert L.ldpc_amd_fec_dgram_unpack_dev(h, *args(B=0)) == 0                                 # nothing to do
    torch.cuda.synchronize()
    assert (by == 0xA5).all() and (off == -1).all() and (st == 0xA5).all()
    assert np.array_equal(d_fr.cpu().numpy(), frames)
    rc, by, off, st = unpack_raw(ctx, d_fr, d_er, k)                         # the context is still usable
    assert rc == 0 and np.array_equal(st.cpu().numpy(), dg.unpack(frames, k, erased)[2])


# ------------------------------------------------------------------------------------------------------------ end to end
def test_datagrams_through_sender_channel_receiver_and_unpack(ctx, oracle):
    code = random_code()
    n, k, S, F = code.n, code.k, 64, 3
    h = ctx.register_code(code)
    oc = oracle.OracleCode(code)
    rng = np.random.default_rng(5)
    N = F * k - 9                                  # the last frame ends with fillers
    ln = np.full(N, S - 4, dtype=np.int64)         # the reference's mix, scaled to S: one short context datagram per 16 full data
    ln[::17] = 12                                  # datagrams, and some of any length
    some = rng.choice(N, size=60, replace=False)
    ln[some] = rng.integers(0, S - 3, size=60)
    off = offsets_of(ln)
    host = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    want_rows = dg.pack(host, off, k, S)

    # the channel, and what it allows: frames 0 and 1 come back whole, frame 2 does not
    drop = np.random.default_rng(5).random((F, n)) < np.array([0.10, 0.10, 0.45])[:, None]   # (the seed: see the two asserts below)
    er_in = drop.astype(np.uint8)
    cw = np.stack([oc.encode(want_rows[f]) for f in range(F)])
    o_er = np.zeros((F, n), dtype=np.uint8)
    for f in range(F):
        o_out, o_er[f], _, _, _ = oc.decode_packets(np.where(drop[f][:, None], 0, cw[f]), er_in[f])
        assert np.array_equal(o_out[~o_er[f].astype(bool)], cw[f][~o_er[f].astype(bool)])
    assert not o_er[0].any() and not o_er[1].any(), "the channel seed must leave frames 0 and 1 decodable"
    assert o_er[2, :k].any() and (drop[2, :k] & ~o_er[2, :k].astype(bool)).any(), "... and frame 2 not, with some source rows recovered"

    # sender: only wire_len[p] bytes of packet p are non-zero
    tx = ctx.fec_tx_device(h, S, block0=254)
    packets, wl = tx.send_datagrams(torch.from_numpy(host).cuda(), off)
    assert tx.next_block == (254 + F) & 0xFF
    assert np.array_equal(wl, dg.wire_len(off, n, k, S))
    pk = packets.cpu().numpy()
    assert pk.shape == (F * n, 8 + S)
    for p in range(F * n):
        assert not pk[p, wl[p]:].any(), p
    assert np.array_equal(pk[:, 8:].reshape(F, n, S), cw)
    # a receive path lands each datagram at stride 8 + S with the tail zeroed
    landed = np.zeros_like(pk)
    for p in range(F * n):
        landed[p, :wl[p]] = pk[p, :wl[p]]
    kept = torch.from_numpy(landed[~drop.reshape(-1)]).cuda()

    with ctx.fec_rx_device(n, k, S) as rx:
        blocks, fr, used = rx.decode_many(h, kept, F)
        last = rx.decode_flush(h)
        assert blocks.tolist() == [254, 255] and used == kept.shape[0] and last is not None and last[0] == 0 and rx.dropped == 0
        frames = torch.cat([fr.out.view(2, n, S), last[1].out.view(1, n, S)]).contiguous()
        er_out = torch.cat([fr.erased_out, last[1].erased_out]).contiguous()
    got = ctx.fec_unpack_datagrams(frames, k, er_out)
    er_out = er_out.cpu().numpy()
    assert np.array_equal(er_out, o_er)
    state, offset, by = got.state.cpu().numpy(), got.offset.cpu().numpy(), got.bytes.cpu().numpy()
    lnr = np.zeros(F * k, dtype=np.int64)
    lnr[:N] = ln
    lost = er_out[:, :k].reshape(-1).astype(bool)
    assert not lost[:2 * k].any() and lost[2 * k:].any()
    assert np.array_equal(state, np.where(lost, dg.LOST, np.where(lnr > 0, dg.DELIVERED, dg.FILLER)))
    assert not (lost & ~drop[:, :k].reshape(-1)).any()            # a received row is never lost
    assert np.array_equal(np.diff(offset), np.where(lost, 0, lnr)) and offset[0] == 0
    # every datagram of frames 0 and 1 byte for byte; of frame 2 every one that was received or recovered
    assert np.array_equal(by[:offset[2 * k]], host[:off[2 * k]])
    for i in range(2 * k, N):
        if not lost[i]:
            assert np.array_equal(by[offset[i]:offset[i + 1]], host[off[i]:off[i + 1]]), i
    assert np.array_equal(by[:offset[-1]], dg.unpack(np.where(o_er.astype(bool)[:, :, None], 0, cw), k, o_er)[0])
