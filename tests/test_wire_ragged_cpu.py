"""The numpy model of the trimmed wire (tools/wire_ragged.py) on the host alone: trim's lengths are the datagram model's
wire_len, land undoes trim, a dropped subset of datagrams lands as the same subset of packets, every way a datagram can be bad
gives the rejected slot, and the host receiver drops those slots and counts them.  Packets come from the host packetiser
(ldpc_amd_fec_packetize) over frames whose source rows tools/datagram_frames.py packed."""
import numpy as np
import pytest

import wire_ragged_cases as cases
from ldpc_erasure_codes_amd import api
from wire_ragged_cases import dg

import wire_ragged as wr  # noqa: E402  (tools/, on the path since wire_ragged_cases)

N_, K_ = 10, 7


@pytest.mark.parametrize("S", [8, 16, 48, 1460])
def test_trim_lengths_are_wire_len_and_land_undoes_trim(S):
    rng = np.random.default_rng(S)
    pk, off = cases.host_packets(rng, 4, N_, K_, S, short=3)
    by, o = wr.trim(pk, K_)
    assert o[0] == 0 and o.dtype == np.int64 and by.shape == (int(o[-1]),)
    assert np.array_equal(np.diff(o), dg.wire_len(off, N_, K_, S))
    for p in (0, K_ - 1, K_, pk.shape[0] - 1):
        assert np.array_equal(by[o[p]:o[p + 1]], pk[p, :o[p + 1] - o[p]])
    back, st = wr.land(by, o, by.shape[0], S)
    assert np.array_equal(back, pk) and (st == wr.LANDED).all()


def test_trim_sends_whole_what_is_no_datagram_symbol():
    S = 16
    pk, _ = cases.host_packets(np.random.default_rng(1), 1, N_, K_, S)
    pk[2, 8:12] = [S - 3, 0, 0, 0]                 # a source row with L = S - 3: whole
    pk[3, 8:12] = [0, 0, 0, 0x80]                  # ... with L = 2^31: whole
    pk[N_ - 1, 8:12] = [1, 0, 0, 0]                # a repair row that reads as L = 1: whole all the same
    pk[4, 8:12] = [S - 4, 0, 0, 0]                 # the longest datagram fills the packet
    pk[5, 8:12] = [2, 0, 0, 0]
    ln = wr.wire_len(pk, K_)
    assert ln[2] == ln[3] == ln[N_ - 1] == ln[4] == 8 + S and ln[5] == 14
    assert wr.wire_len(pk, 5)[5] == 8 + S and wr.wire_len(pk, 6)[5] == 14      # k decides what a source row is
    by, o = wr.trim(pk, K_)
    assert np.array_equal(by[o[5]:o[6]], pk[5, :14]) and np.array_equal(by[o[2]:o[3]], pk[2])


def test_a_dropped_subset_lands_as_the_same_subset():
    S = 48
    rng = np.random.default_rng(2)
    pk, _ = cases.host_packets(rng, 5, N_, K_, S)
    by, o = wr.trim(pk, K_)
    keep = rng.random(pk.shape[0]) >= 0.3
    by2 = np.concatenate([by[o[p]:o[p + 1]] for p in np.nonzero(keep)[0]])
    o2 = np.concatenate([[0], np.cumsum(np.diff(o)[keep])])
    back, st = wr.land(by2, o2, by2.shape[0], S)
    assert 0 < keep.sum() < keep.shape[0]
    assert np.array_equal(back, pk[keep]) and (st == wr.LANDED).all()


def test_every_rejected_condition_gives_the_ff_header_and_zeros():
    S = 16
    rng = np.random.default_rng(3)
    pk, _ = cases.host_packets(rng, 3, N_, K_, S)
    by, o = wr.trim(pk, K_)
    data = np.concatenate([by, rng.integers(0, 256, size=64, dtype=np.uint8)])
    nbytes = by.shape[0] + 40            # the two planted tails lie inside the buffer: their LENGTH is what is wrong
    o2, kinds = cases.plant_bad(o, nbytes, S)
    o2, far = cases.plant_far(o2)
    kinds.update(far)
    back, st = wr.land(data, o2, nbytes, S)
    slot = np.zeros(8 + S, dtype=np.uint8)
    slot[:8] = 0xFF
    for kind, p in kinds.items():
        assert st[p] == wr.REJECTED and np.array_equal(back[p], slot), kind
    w_back, w_st = cases.land_scalar(data, o2, nbytes, S)
    assert np.array_equal(st, w_st) and np.array_equal(back, w_back)
    assert (back[st == wr.REJECTED] == slot).all()
    same = [p for p in range(pk.shape[0]) if o2[p] == o[p] and o2[p + 1] == o[p + 1]]
    assert len(same) > 10 and (st[same] == wr.LANDED).all() and np.array_equal(back[same], pk[same])
    # the limits themselves land: 8 bytes and 8 + S bytes, ending exactly at nbytes
    edge = np.array([0, 8, 8 + 8 + S], dtype=np.int64)
    back, st = wr.land(data, edge, 16 + S, S)
    assert (st == wr.LANDED).all() and np.array_equal(back[0, :8], data[:8]) and not back[0, 8:].any()
    assert np.array_equal(back[1], data[8:16 + S])
    assert wr.land(data, edge, 16 + S - 1, S)[1].tolist() == [wr.LANDED, wr.REJECTED]
    # nothing to read at all: every datagram is rejected
    back, st = wr.land(np.zeros(0, dtype=np.uint8), np.array([0, 0, 0]), 0, S)
    assert (st == wr.REJECTED).all() and (back[:, :8] == 0xFF).all() and not back[:, 8:].any()
    with pytest.raises(ValueError):
        wr.land(data, o, nbytes, 10)


def test_the_host_receiver_drops_rejected_slots_and_counts_them():
    S = 16
    rng = np.random.default_rng(4)
    pk, _ = cases.host_packets(rng, 2, N_, K_, S)
    P = pk.shape[0]
    by, o = wr.trim(pk, K_)
    o2, kinds = cases.plant_bad(o, by.shape[0], S)
    landed, st = wr.land(by, o2, by.shape[0], S)
    bad = st == wr.REJECTED
    assert not bad[0]                    # (a receiver takes its first block number from the first packet it sees, dropped or not)
    assert api.fec_header_unpack(int(landed[bad][0, :8].copy().view("<u8")[0]))[2] == 0xFFFF
    same = np.zeros(landed.shape[0], dtype=bool)
    same[:P] = (o2[:P] == o[:P]) & (o2[1:P + 1] == o[1:P + 1])          # the datagrams that arrived as they were sent
    assert not (same & bad).any() and np.array_equal(landed[same], pk[same[:P]])

    rx, ref = api.FecRx(N_, K_, S), api.FecRx(N_, K_, S)
    got = rx.push_many(landed[same | bad], 3)
    want = ref.push_many(pk[same[:P]], 3)                                # the same stream without the rejected slots
    assert int(bad.sum()) >= len(set(kinds.values())) == 7
    assert rx.dropped == ref.dropped + int(bad.sum())                    # (both drop what belongs to neither open block)
    assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    blocks = got[0].tolist()
    while True:
        a, b = rx.flush(), ref.flush()
        assert (a is None) == (b is None)
        if a is None:
            break
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert not a[2].all()                                            # the block did receive packets
        blocks.append(a[0])
    assert blocks == [254, 255]
    rx.close()
    ref.close()
