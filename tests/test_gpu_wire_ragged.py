"""GPU tests of the trimmed wire (include/ldpc_erasure_amd_wire_ragged.h, csrc/wire_ragged_dev.hip): trim and land against the numpy
model tools/wire_ragged.py byte for byte, loop-back on the device, a packet array beyond 2^32 bytes, the refusals, and datagrams of
mixed lengths through sender, trim, a lossy ragged wire, land, receiver and unpack against the fixed-stride path, single-flow and
multi-flow.  Every buffer of the byte-for-byte tests lies between 4 KiB sentinel bands; outputs are pre-filled with a poison byte."""
import numpy as np
import pytest

import wire_ragged_cases as cases
from code_helpers import random_code
from ldpc_erasure_codes_amd import api
from wire_ragged_cases import dg

import wire_ragged as wr  # noqa: E402  (tools/, on the path since wire_ragged_cases)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_word_symbols import Arena  # noqa: E402  (4 KiB sentinel bands around every buffer)

EINVAL, EUNSUP = -1, -5
POISON = 0xEE
N_, K_ = 10, 7
TILE = 256          # packets per tile of the trim scan (kTile of wire_ragged_dev.hip)
SCAN_ROUND = 1024   # tile sums one round of the scan workgroup's loop takes (kThreads * kScanPer)
GIB = 1 << 30
SIZES = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
# The end-to-end channel removes a seeded 10 % of the datagrams.  A code that always decodes at 10 % would make the comparison of the
# two paths vacuous, so the code is a weak one (24 checks for 224 symbols) and the seed one for which -- on the fixed-stride path, the
# code as it was before trim and land existed -- some dropped source rows come back and some stay lost (asserted in the test).
WEAK = dict(n=224, k=200, coldeg=1, seed=3)
CHANNEL_SEED = 6


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
    return bool((t.view(-1).view(torch.uint8) == POISON).all())


def shuffled_packets(rng, P, S, plant=True):
    """P packets out of frame order (as ROUND_ROBIN output is): pack-made source rows of every edge length, noise repair rows, the
    host packetiser, a permutation; a few source rows get a planted L > S - 4."""
    pk, _ = cases.host_packets(rng, -(-P // N_) + 1, N_, K_, S, short=2)
    pk = pk[rng.permutation(pk.shape[0])[:P]].copy()
    if plant and P >= TILE - 1:
        src = np.nonzero((pk[:, 0].astype(int) | pk[:, 1].astype(int) << 8) < K_)[0]
        for j, p in enumerate(rng.choice(src, size=6, replace=False)):
            pk[p, 8:12] = np.frombuffer(np.uint32([S - 3, 0xFFFFFFFF, S, 1 << 31, S + 4, 0x01000000][j]).astype("<u4").tobytes(), dtype=np.uint8)
    return pk


def trim_raw(ctx, pk, P, k, S, by, cap, off):
    ptr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()   # noqa: E731
    return ctx._L.ldpc_amd_fec_wire_trim_dev(ctx._h, ptr(pk), P, k, S, ptr(by), cap, ptr(off))


def land_raw(ctx, data, nbytes, off, P, S, pk, st):
    ptr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()   # noqa: E731
    return ctx._L.ldpc_amd_fec_wire_land_dev(ctx._h, ptr(data), nbytes, ptr(off), P, S, ptr(pk), ptr(st))


def check_trim(ctx, pk, k):
    """Trim of the host array pk on guarded, poisoned buffers against the model; returns the model's (bytes, offset)."""
    P, plen = pk.shape
    arn = Arena()
    d_pk = arn.new(pk.shape, src=pk)
    by = poisoned(arn, (P * plen,))
    off = poisoned(arn, (P + 1,), torch.int64)
    rc = trim_raw(ctx, d_pk, P, k, plen - 8, by, P * plen, off)
    assert rc == 0, ctx._L.ldpc_amd_last_error(ctx._h)
    arn.check()
    w_by, w_off = wr.trim(pk, k)
    total = int(w_off[-1])
    assert np.array_equal(off.cpu().numpy(), w_off)
    got = by.cpu().numpy()
    assert np.array_equal(got[:total], w_by)
    assert (got[total:] == POISON).all()           # nothing at or beyond the total is written
    assert np.array_equal(d_pk.cpu().numpy(), pk)
    return w_by, w_off


# ------------------------------------------------------------------------------------------------------------------ trim
@pytest.mark.parametrize("S", [8, 16, 48, 1460])
@pytest.mark.parametrize("P", SIZES)
def test_trim_is_the_models_bytes_at_every_destination_phase(ctx, S, P):
    rng = np.random.default_rng(1000 * S + P)
    pk = shuffled_packets(rng, P, S)
    sym = pk[:, 0].astype(int) | pk[:, 1].astype(int) << 8
    _, w_off = check_trim(ctx, pk, K_)
    if P > 1:
        assert (np.diff(sym) != 1).any() and (sym < K_).any() and (sym >= K_).any()      # out of frame order, both kinds of row
        assert {int(o % 4) for o in w_off[:-1]} == {0, 1, 2, 3}                          # (the arena's buffers are 16-byte aligned)
        whole_src = (sym < K_) & (np.diff(w_off) == 8 + S) & (np.ascontiguousarray(pk[:, 8:12]).view("<u4")[:, 0] != S - 4)
        assert whole_src.any() == (P >= TILE - 1), "planted source rows that are no datagram symbols are sent whole"
    assert ctx.fec_wire_ragged_info()["trim_packets"] == P
    # the pack-made case, in frame order: the lengths are ldpc_amd_fec_dgram_wire_len's, entry for entry
    pk0, dgoff = cases.host_packets(rng, 3, N_, K_, S, short=2)
    _, w_off0 = check_trim(ctx, pk0, K_)
    assert np.array_equal(np.diff(w_off0), api.fec_datagram_wire_len(dgoff, N_, K_, S))


def test_trim_when_the_tile_sum_scan_crosses_its_round(ctx):
    S, P = 8, SCAN_ROUND * TILE + 300
    assert -(-P // TILE) > SCAN_ROUND
    rng = np.random.default_rng(77)
    F = -(-P // N_)
    ln = rng.integers(0, S - 3, size=F * K_)
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    frames = rng.integers(0, 256, size=(F, N_, S), dtype=np.uint8)
    frames[:, :K_] = dg.pack(rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8), off, K_, S)
    pk = api.fec_packetize(frames)[:P]
    check_trim(ctx, pk, K_)


def test_trim_through_the_binding_and_its_info(ctx):
    rng = np.random.default_rng(5)
    pk = shuffled_packets(rng, 300, 48)
    w = ctx.fec_trim_packets(torch.from_numpy(pk).cuda(), K_)
    assert isinstance(w, api.Wire) and w.bytes.shape == (300 * 56,) and w.offset.shape == (301,) and w.offset.dtype == torch.int64
    w_by, w_off = wr.trim(pk, K_)
    assert np.array_equal(w.offset.cpu().numpy(), w_off) and np.array_equal(w.bytes[:int(w_off[-1])].cpu().numpy(), w_by)
    info = ctx.fec_wire_ragged_info()
    assert info["trim_packets"] == 300 and info["scratch_bytes"] >= 8 * 2 + 4 * 300
    ctx.fec_land_packets(w.bytes, w.offset, 48)
    assert ctx.fec_wire_ragged_info()["land_packets"] == 300
    empty = ctx.fec_trim_packets(torch.zeros((0, 56), dtype=torch.uint8, device="cuda"), K_)
    assert empty.bytes.shape == (0,) and empty.offset.tolist() == [0]
    assert ctx.fec_wire_ragged_info()["trim_packets"] == 300          # no packets: nothing was touched


# ------------------------------------------------------------------------------------------------------------------ land
def ragged_stream(rng, P, S):
    """(data, offsets, nbytes, planted kinds): P datagrams of lengths 8, 9, 11, 12, 8 + S - 1, 8 + S mixed with random ones, random
    bytes, and -- from 255 datagrams on -- every REJECTED kind planted, offsets far outside the buffer among them."""
    pool = [8, 9, 11, 12, 8 + S - 1, 8 + S]
    ln = np.array([int(rng.choice(pool)) if rng.random() < 0.5 else int(rng.integers(8, 8 + S + 1)) for _ in range(P)], dtype=np.int64)
    first = int(rng.integers(0, 8))
    o = np.concatenate([[first], first + np.cumsum(ln)]).astype(np.int64)
    nbytes = int(o[-1]) + 40
    kinds = {}
    if P >= TILE - 1:
        nbytes = int(o[-3]) + 7 + 8 + S + 1 + 40            # (plant_bad appends two datagrams; they lie inside the buffer)
        o, kinds = cases.plant_bad(o[:-2], nbytes, S)
        o, far = cases.plant_far(o)
        kinds.update(far)
        assert o.shape[0] == P + 1
    return rng.integers(0, 256, size=nbytes, dtype=np.uint8), o, nbytes, kinds


@pytest.mark.parametrize("S", [8, 16, 48, 1460])
@pytest.mark.parametrize("P", SIZES)
def test_land_is_the_models_bytes_at_every_source_phase(ctx, S, P):
    rng = np.random.default_rng(2000 * S + P)
    data, o, nbytes, kinds = ragged_stream(rng, P, S)
    w_pk, w_st = wr.land(data, o, nbytes, S)
    s_pk, s_st = cases.land_scalar(data, o, nbytes, S)
    assert np.array_equal(w_pk, s_pk) and np.array_equal(w_st, s_st)
    slot = np.zeros(8 + S, dtype=np.uint8)
    slot[:8] = 0xFF
    for kind, p in kinds.items():
        assert w_st[p] == wr.REJECTED and np.array_equal(w_pk[p], slot), kind
    assert (w_st == wr.LANDED).any() and ((w_st == wr.REJECTED).sum() >= 11) == (P >= TILE - 1)
    phases = set()
    for start in (0, 1, 2, 3):
        arn = Arena()
        base = arn.new((start + nbytes,))
        base[start:] = torch.from_numpy(data).cuda()
        d_data = base[start:]                      # `data` starts `start` bytes into its buffer
        assert d_data.data_ptr() % 4 == start
        phases |= {int((d_data.data_ptr() + a) % 4) for a, s in zip(o[:-1], w_st) if s == wr.LANDED}
        d_off = arn.new((P + 1,), torch.int64, src=o)
        pk, st = poisoned(arn, (P, 8 + S)), poisoned(arn, (P,))
        assert land_raw(ctx, d_data, nbytes, d_off, P, S, pk, st) == 0, ctx._L.ldpc_amd_last_error(ctx._h)
        pk2 = poisoned(arn, (P, 8 + S))
        assert land_raw(ctx, d_data, nbytes, d_off, P, S, pk2, None) == 0       # without a state array: the same packets
        arn.check()                                # the bands around data, the offsets, the packets and the states are intact
        assert np.array_equal(st.cpu().numpy(), w_st), (S, P, start)
        assert np.array_equal(pk.cpu().numpy(), w_pk), (S, P, start)
        assert torch.equal(pk2, pk)
        assert np.array_equal(base[start:].cpu().numpy(), data) and np.array_equal(d_off.cpu().numpy(), o)
    assert phases == {0, 1, 2, 3}
    assert ctx.fec_wire_ragged_info()["land_packets"] == P


def test_land_with_nothing_to_read_rejects_everything(ctx):
    arn = Arena()
    S, P = 16, 5
    d_off = arn.new((P + 1,), torch.int64, src=np.array([0, 0, 8, 30, -4, 0], dtype=np.int64))
    pk, st = poisoned(arn, (P, 8 + S)), poisoned(arn, (P,))
    assert land_raw(ctx, None, 0, d_off, P, S, pk, st) == 0
    arn.check()
    assert (st == wr.REJECTED).all() and bool((pk[:, :8] == 0xFF).all()) and not bool(pk[:, 8:].any())
    assert land_raw(ctx, None, 0, d_off, 0, S, None, None) == 0                  # no datagrams: nothing to do


# ------------------------------------------------------------------------------------------------------------- loop-back
def datagram_mix(rng, N, S):
    """The reference's mix scaled to S (one short context datagram per 16 full data datagrams) and some of any length."""
    ln = np.full(N, S - 4, dtype=np.int64)
    ln[::17] = 12
    some = rng.choice(N, size=N // 4, replace=False)
    ln[some] = rng.integers(0, S - 3, size=some.shape[0])
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    return rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8), off


def test_loop_back_on_the_device(ctx):
    code = random_code()
    n, k, S = code.n, code.k, 64
    h = ctx.register_code(code)
    rng = np.random.default_rng(8)
    host, off = datagram_mix(rng, 2 * k - 9, S)
    pk, wl = ctx.fec_tx_device(h, S, block0=255).send_datagrams(torch.from_numpy(host).cuda(), off)
    w = ctx.fec_trim_packets(pk, k)
    assert torch.equal(w.offset[1:] - w.offset[:-1], torch.from_numpy(wl.astype(np.int64)).cuda())
    back, st = ctx.fec_land_packets(w.bytes, w.offset, S)
    assert torch.equal(back, pk) and not bool(st.any())
    # three flows, one packet of every flow in turn
    nf, per = 3, 2
    host, off = datagram_mix(rng, nf * per * k, S)
    src = ctx.fec_pack_datagrams(torch.from_numpy(host).cuda(), off, k, S)
    pk, flow_of, _ = ctx.fec_tx_flows(h, S, nf, block0=[0, 100, 254]).send(src, np.arange(nf + 1) * per, api.TX_ROUND_ROBIN)
    sym = pk[:, 0].to(torch.int64) | pk[:, 1].to(torch.int64) << 8
    assert bool((sym[1:] - sym[:-1] != 1).any())
    w = ctx.fec_trim_packets(pk, k)
    assert int(w.offset[-1]) < pk.numel() and int(w.offset[-1]) == int(torch.where(sym < k, 12 + pk[:, 8].to(torch.int64), 8 + S).sum())
    back, st = ctx.fec_land_packets(w.bytes, w.offset, S)
    assert torch.equal(back, pk) and not bool(st.any())


def test_beyond_two_to_the_32(ctx):
    S, k = 1460, K_
    plen = 8 + S
    P = int(1.06 * (1 << 32)) // plen
    need = 3 * P * plen + (2 << 30)           # the packets, the wire bytes, the landed packets; offsets, lengths and the index below 2 GiB
    assert P * plen > 1 << 32 and need < 16 * GIB
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need / GIB:.1f} GiB of device memory, {free / GIB:.1f} GiB free")
    rng = np.random.default_rng(9)
    small, _ = cases.host_packets(rng, 101, N_, K_, S)                    # 1010 packets: no power of two is a multiple
    small[:, 8:12][(small[:, 0] < K_) & (rng.random(small.shape[0]) < 0.95)] = np.frombuffer(np.uint32(S - 4).astype("<u4").tobytes(), dtype=np.uint8)
    M = small.shape[0]
    idx = torch.arange(P, device="cuda") % M
    pk = torch.from_numpy(small).cuda().index_select(0, idx)
    ln = torch.from_numpy(wr.wire_len(small, k)).cuda().index_select(0, idx)
    del idx
    w = ctx.fec_trim_packets(pk, k)
    want = torch.cumsum(ln, 0)
    assert int(want[-1]) > 1 << 32
    assert int(w.offset[0]) == 0 and torch.equal(w.offset[1:], want)
    del want, ln
    back, st = ctx.fec_land_packets(w.bytes, w.offset, S)
    assert not bool(st.any())
    step = 1 << 18
    for p0 in range(0, P, step):
        assert torch.equal(back[p0:p0 + step], pk[p0:p0 + step]), p0
    # the wire bytes themselves, where the byte address passes 2^32: the packet that straddles it and the last one
    off = w.offset
    for p in (int(torch.searchsorted(off, torch.tensor([1 << 32], device="cuda"))[0]) - 1, P - 1):
        a, b = int(off[p]), int(off[p + 1])
        assert torch.equal(w.bytes[a:b], pk[p, :b - a]), p
    del w, back, pk
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ end to end
def drop_from_the_wire(w, keep):
    """The wire bytes come back to the host, the datagrams with keep == False are removed in numpy, the rest goes back up."""
    o = w.offset.cpu().numpy()
    by = w.bytes.cpu().numpy()[:o[-1]]
    ln = np.diff(o)
    return by[np.repeat(keep, ln)], np.concatenate([[0], np.cumsum(ln[keep])]).astype(np.int64)


def receive_single(ctx, h, n, k, S, packets, F):
    """decode_many + decode_flush until the stream is empty + unpack -> everything the receiver says, on the host."""
    with ctx.fec_rx_device(n, k, S) as rx:
        blocks, fr, used = rx.decode_many(h, packets, F)
        blocks, frs = blocks.tolist(), [fr]
        while True:
            last = rx.decode_flush(h)
            if last is None:
                break
            blocks.append(last[0])
            frs.append(last[1])
        dropped = rx.dropped
    fr = api.DecodedFrames(*(torch.cat([getattr(f, name) for f in frs]).contiguous() for name in api.DecodedFrames._fields))
    got = ctx.fec_unpack_datagrams(fr.out.view(-1, n, S), k, fr.erased_out)
    total = int(got.offset[-1])
    return dict(blocks=blocks, used=used, dropped=dropped, out=fr.out.cpu().numpy(), erased_out=fr.erased_out.cpu().numpy(),
                sweeps=fr.sweeps.cpu().numpy(), residual=fr.residual.cpu().numpy(), status=fr.status.cpu().numpy(),
                residual_src=fr.residual_src.cpu().numpy(), state=got.state.cpu().numpy(), offset=got.offset.cpu().numpy(),
                bytes=got.bytes[:total].cpu().numpy())


def same_results(a, b, skip=()):
    for key in a:
        if key in skip:
            continue
        assert np.array_equal(a[key], b[key]), key


def test_end_to_end_against_the_fixed_stride_path(ctx):
    code = random_code(**WEAK)
    n, k, S, F, b0 = code.n, code.k, 64, 4, 254
    h = ctx.register_code(code)
    rng = np.random.default_rng(10)
    host, off = datagram_mix(rng, F * k - 9, S)
    data = torch.from_numpy(host).cuda()
    keep = np.random.default_rng(CHANNEL_SEED).random(F * n) >= 0.10
    # the path that exists without trim and land: fixed-stride packets, the survivors picked by index
    pk, wl = ctx.fec_tx_device(h, S, block0=b0).send_datagrams(data, off)
    fixed = receive_single(ctx, h, n, k, S, pk.index_select(0, torch.from_numpy(np.nonzero(keep)[0]).cuda()), F)
    frame_of = [(b - b0) & 0xFF for b in fixed["blocks"]]
    assert len(frame_of) >= 2 and all(f < F for f in frame_of)
    dropped_src = np.concatenate([~keep.reshape(F, n)[f, :k] for f in frame_of])
    came_back = int((dropped_src & (fixed["state"] == dg.DELIVERED)).sum())
    lost = int((fixed["state"] == dg.LOST).sum())
    assert came_back > 0 and lost > 0, (came_back, lost)
    # the trimmed path: ragged wire bytes, the same datagrams removed from the stream, landed
    tx = ctx.fec_tx_device(h, S, block0=b0)
    w = tx.send_datagrams_trimmed(data, off)
    assert tx.next_block == (b0 + F) & 0xFF
    assert np.array_equal(np.diff(w.offset.cpu().numpy()), wl)
    by, o = drop_from_the_wire(w, keep)
    assert by.shape[0] < int(keep.sum()) * (8 + S)
    landed, st = ctx.fec_land_packets(torch.from_numpy(by).cuda(), torch.from_numpy(o).cuda(), S)
    assert not bool(st.any())
    trimmed = receive_single(ctx, h, n, k, S, landed, F)
    same_results(fixed, trimmed)


def receive_mixed(ctx, h, nf, n, k, S, packets, flow_of, per):
    with ctx.fec_rx_flows(nf, n, k, S) as rx:
        closes, blocks, fr, consumed, offered = rx.decode_mixed(h, packets, flow_of, per + 2)
        res = dict(closes=closes, blocks=blocks, consumed=consumed, offered=offered)
        frs = [fr]
        for f in range(nf):
            while True:
                last = rx.decode_flush(f, h)
                if last is None:
                    break
                res[f"flush {f} {len(frs)}"] = np.array(last[0])
                frs.append(last[1])
        res["dropped"] = rx.dropped
    fr = api.DecodedFrames(*(torch.cat([getattr(f, name) for f in frs]).contiguous() for name in api.DecodedFrames._fields))
    got = ctx.fec_unpack_datagrams(fr.out.view(-1, n, S), k, fr.erased_out)
    res.update(out=fr.out.cpu().numpy(), erased_out=fr.erased_out.cpu().numpy(), sweeps=fr.sweeps.cpu().numpy(), residual=fr.residual.cpu().numpy(),
               status=fr.status.cpu().numpy(), residual_src=fr.residual_src.cpu().numpy(), state=got.state.cpu().numpy(),
               offset=got.offset.cpu().numpy(), bytes=got.bytes[:int(got.offset[-1])].cpu().numpy())
    return res


def test_end_to_end_many_flows_with_a_rejected_datagram(ctx):
    code = random_code(**WEAK)
    n, k, S, nf, per = code.n, code.k, 64, 3, 2
    h = ctx.register_code(code)
    rng = np.random.default_rng(11)
    host, off = datagram_mix(rng, nf * per * k, S)
    src = ctx.fec_pack_datagrams(torch.from_numpy(host).cuda(), off, k, S)
    block0, begin = [250, 0, 255], np.arange(nf + 1) * per
    pk, flow_of, _ = ctx.fec_tx_flows(h, S, nf, block0=block0).send(src, begin, api.TX_ROUND_ROBIN)
    P = pk.shape[0]
    keep = np.random.default_rng(CHANNEL_SEED + 1).random(P) >= 0.10
    kept = torch.from_numpy(np.nonzero(keep)[0]).cuda()
    fixed = receive_mixed(ctx, h, nf, n, k, S, pk.index_select(0, kept), flow_of.index_select(0, kept), per)
    assert (fixed["state"] == dg.DELIVERED).any() and int(fixed["offered"].sum()) == int(keep.sum())
    # the trimmed wire, with a runt of 5 bytes that claims to be of flow 1 in the middle of the stream
    w = ctx.fec_trim_packets(pk, k)
    by, o = drop_from_the_wire(w, keep)
    at, runt_flow = o.shape[0] // 2, 1
    by = np.concatenate([by[:o[at]], np.full(5, 0x5A, dtype=np.uint8), by[o[at]:]])
    o = np.concatenate([o[:at + 1], o[at:] + 5])
    fo = flow_of.cpu().numpy()[keep]
    fo = np.concatenate([fo[:at], [runt_flow], fo[at:]]).astype(np.int32)
    landed, st = ctx.fec_land_packets(torch.from_numpy(by).cuda(), torch.from_numpy(o).cuda(), S)
    st = st.cpu().numpy()
    assert st[at] == api.WIRE_REJECTED and st.sum() == 1
    assert bool((landed[at, :8] == 0xFF).all()) and not bool(landed[at, 8:].any())
    assert torch.equal(landed[at + 1], pk[int(np.nonzero(keep)[0][at])])
    trimmed = receive_mixed(ctx, h, nf, n, k, S, landed, torch.from_numpy(fo).cuda(), per)
    same_results(fixed, trimmed, skip=("dropped", "offered", "consumed"))
    extra = np.zeros(nf, dtype=np.int64)
    extra[runt_flow] = 1
    assert np.array_equal(trimmed["dropped"], fixed["dropped"] + extra)      # the rejected slot shows up in its flow's count
    assert np.array_equal(trimmed["offered"], fixed["offered"] + extra) and np.array_equal(trimmed["consumed"], fixed["consumed"] + extra)


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_every_output_as_poison(ctx):
    rng = np.random.default_rng(12)
    S, P = 16, 40
    plen = 8 + S
    pk_h = shuffled_packets(rng, P, S, plant=False)
    w_by, w_off = wr.trim(pk_h, K_)
    arn = Arena()
    d_pk = arn.new(pk_h.shape, src=pk_h)
    by, off = poisoned(arn, (P * plen,)), poisoned(arn, (P + 1,), torch.int64)
    d_data = arn.new(w_by.shape, src=w_by)
    d_off = arn.new(w_off.shape, torch.int64, src=w_off)
    out, st = poisoned(arn, (P, plen)), poisoned(arn, (P,))
    host_pk, host_off = pk_h.copy(), w_off.copy()
    L, hnd = ctx._L, ctx._h
    err = lambda: L.ldpc_amd_last_error(hnd)   # noqa: E731

    def trim(**kw):
        a = dict(pk=d_pk.data_ptr(), P=P, k=K_, S=S, by=by.data_ptr(), cap=P * plen, off=off.data_ptr())
        a.update(kw)
        return trim_raw(ctx, a["pk"], a["P"], a["k"], a["S"], a["by"], a["cap"], a["off"])

    def land(**kw):
        a = dict(data=d_data.data_ptr(), nbytes=w_by.shape[0], off=d_off.data_ptr(), P=P, S=S, pk=out.data_ptr(), st=st.data_ptr())
        a.update(kw)
        return land_raw(ctx, a["data"], a["nbytes"], a["off"], a["P"], a["S"], a["pk"], a["st"])

    assert trim(S=10) == EUNSUP and trim(S=4) == EUNSUP and b"multiple of 4" in err()
    assert trim(cap=P * plen - 1) == EINVAL and b"cap" in err()
    assert trim(P=-1) == EINVAL and trim(P=1 << 31) == EINVAL
    assert trim(k=0) == EINVAL
    assert trim(pk=host_pk.ctypes.data) == EINVAL and b"device pointers" in err()                 # host memory
    assert trim(off=host_off.ctypes.data) == EINVAL
    assert trim(pk=None) == EINVAL and trim(by=None) == EINVAL and trim(off=None) == EINVAL
    assert trim(pk=d_pk.data_ptr() + 2, P=P - 1, cap=(P - 1) * plen) == EINVAL and b"aligned" in err()
    assert trim(off=off.data_ptr() + 4, P=P - 1, cap=(P - 1) * plen) == EINVAL
    assert trim(by=d_pk.data_ptr(), cap=P * plen) == EINVAL and b"overlaps" in err()             # bytes_out over the packets
    assert trim(off=by.data_ptr() + 8) == EINVAL                                                   # offset_out inside bytes_out
    assert trim(P=0) == 0                                                                          # nothing to do

    assert land(S=10) == EUNSUP and land(S=4) == EUNSUP
    assert land(P=-1) == EINVAL and land(nbytes=-1) == EINVAL and land(P=1 << 31) == EINVAL
    assert land(data=None) == EINVAL and b"NULL" in err()                                          # NULL bytes with nbytes > 0
    assert land(data=w_by.ctypes.data) == EINVAL and land(off=host_off.ctypes.data) == EINVAL      # host memory
    assert land(off=None) == EINVAL and land(pk=None) == EINVAL
    assert land(pk=out.data_ptr() + 2, P=P - 1) == EINVAL and land(off=d_off.data_ptr() + 4, P=P - 1) == EINVAL
    assert land(pk=d_data.data_ptr()) == EINVAL                                                    # packets over the wire bytes
    assert land(st=out.data_ptr() + 8) == EINVAL and land(st=d_off.data_ptr()) == EINVAL           # state over packets / offsets
    assert land(pk=d_off.data_ptr() & ~3, P=1) == EINVAL
    assert land(P=0) == 0
    with pytest.raises(api.LdpcAmdError, match="multiple of 4"):
        ctx.fec_land_packets(d_data, d_off, 10)
    arn.check()
    for t in (by, off, out, st):
        assert is_poison(t)
    assert np.array_equal(d_pk.cpu().numpy(), pk_h) and np.array_equal(d_data.cpu().numpy(), w_by) and np.array_equal(d_off.cpu().numpy(), w_off)
    # the context is still usable
    assert trim() == 0 and land() == 0
    arn.check()
    assert np.array_equal(off.cpu().numpy(), w_off) and np.array_equal(by.cpu().numpy()[:w_off[-1]], w_by)
    assert np.array_equal(out.cpu().numpy(), pk_h) and not bool(st.any())
