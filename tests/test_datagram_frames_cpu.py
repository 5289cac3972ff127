"""tools/datagram_frames.py, the numpy statement of the datagram symbol format (include/ldpc_erasure_amd_datagrams.h) and the
yardstick of tests/test_gpu_datagrams.py, checked on the host alone: unpack undoes pack, lost rows are skipped with dense offsets,
a malformed prefix is flagged and not copied."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import datagram_frames as dg  # noqa: E402


def random_datagrams(rng, N, S, special=True):
    pool = [0, 1, 2, 3, 4, 5, S - 5, S - 4] if special else []
    ln = np.array([int(rng.choice(pool)) if pool and rng.random() < 0.5 else int(rng.integers(0, S - 3)) for _ in range(N)], dtype=np.int64)
    ln = np.clip(ln, 0, S - 4)
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    return rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8), off


@pytest.mark.parametrize("S", [8, 16, 48, 1460])
@pytest.mark.parametrize("N", [0, 1, 6, 7, 8, 38])
def test_unpack_undoes_pack(S, N):
    rng = np.random.default_rng(S * 100 + N)
    k = 7
    data, off = random_datagrams(rng, N, S)
    src = dg.pack(data, off, k, S)
    F = -(-N // k)
    assert src.shape == (F, k, S)
    rows = src.reshape(F * k, S)
    ln = np.diff(off)
    for i in range(F * k):
        L = int(ln[i]) if i < N else 0
        assert rows[i, :4].tolist() == [L & 255, (L >> 8) & 255, (L >> 16) & 255, L >> 24]   # little-endian
        assert np.array_equal(rows[i, 4:4 + L], data[off[i]:off[i] + L]) if i < N else True
        assert not rows[i, 4 + L:].any()
    # as frames of n = k + 3 rows whose repair rows are noise
    frames = rng.integers(0, 256, size=(F, k + 3, S), dtype=np.uint8)
    frames[:, :k] = src
    by, o, st = dg.unpack(frames, k)
    assert np.array_equal(by, data)
    want_len = np.zeros(F * k, dtype=np.int64)
    want_len[:N] = ln
    assert np.array_equal(np.diff(o), want_len) and o[0] == 0 and o[-1] == data.shape[0]
    assert np.array_equal(st, np.where(want_len > 0, dg.DELIVERED, dg.FILLER))


def test_lost_rows_are_skipped_and_offsets_stay_dense():
    rng = np.random.default_rng(5)
    k, n, S, N = 5, 8, 32, 20
    data, off = random_datagrams(rng, N, S, special=False)
    src = dg.pack(data, off, k, S)
    frames = np.zeros((4, n, S), dtype=np.uint8)
    frames[:, :k] = src
    erased = (rng.random((4, n)) < 0.4).astype(np.uint8)
    frames[erased.astype(bool)] = 0xEE   # what an erased row holds does not matter, its prefix is not looked at
    by, o, st = dg.unpack(frames, k, erased)
    ln = np.diff(off)
    lost = erased[:, :k].reshape(-1).astype(bool)
    assert lost.any() and not lost.all()
    assert np.array_equal(st[lost], np.full(int(lost.sum()), dg.LOST))
    assert np.array_equal(st[~lost], np.where(ln[~lost] > 0, dg.DELIVERED, dg.FILLER))
    assert np.array_equal(np.diff(o), np.where(lost, 0, ln))
    assert np.array_equal(by, np.concatenate([data[off[i]:off[i + 1]] for i in range(N) if not lost[i]]))


@pytest.mark.parametrize("bad", ["S-3", "0xFFFFFFFF"])
def test_malformed_prefix_is_flagged_and_not_copied(bad):
    k, n, S = 3, 4, 16
    data = np.arange(1, 25, dtype=np.uint8)
    frames = np.zeros((1, n, S), dtype=np.uint8)
    frames[0, :k] = dg.pack(data, [0, 12, 12 + 5, 24], k, S)[0]
    L = S - 3 if bad == "S-3" else 0xFFFFFFFF
    frames[0, 1, :4] = np.frombuffer(np.uint32(L).astype("<u4").tobytes(), dtype=np.uint8)
    by, o, st = dg.unpack(frames, k)
    assert st.tolist() == [dg.DELIVERED, dg.MALFORMED, dg.DELIVERED]
    assert o.tolist() == [0, 12, 12, 19]
    assert np.array_equal(by, np.concatenate([data[:12], data[17:]]))


def test_pack_refuses_what_the_format_cannot_hold():
    with pytest.raises(ValueError):
        dg.pack(np.zeros(64, dtype=np.uint8), [0, 13], 2, 16)      # S - 3 bytes
    with pytest.raises(ValueError):
        dg.pack(np.zeros(64, dtype=np.uint8), [0, 8, 4], 2, 16)    # decreasing
    with pytest.raises(ValueError):
        dg.pack(np.zeros(64, dtype=np.uint8), [0, 4], 2, 10)       # S not a multiple of 4


def test_wire_len_and_difi_mix():
    rng = np.random.default_rng(1)
    S, k, n = 1024, 20, 30
    data, off = dg.difi_mix(rng, 35, S)
    ln = np.diff(off)
    assert ln[0] == 112 and ln[17] == 112 and ln[34] == 112 and (np.delete(ln, [0, 17, 34]) == S - 4).all()
    assert data.shape[0] == off[-1]
    w = dg.wire_len(off, n, k, S).reshape(2, n)
    assert (w[:, k:] == 8 + S).all()
    assert np.array_equal(w[:, :k].reshape(-1)[:35], 12 + ln) and (w[1, 15:k] == 12).all()
    # everything behind wire_len is zero in a packet whose payload is the row
    rows = dg.pack(data, off, k, S).reshape(-1, S)
    for r in (0, 1, 17, 35, 39):
        assert not rows[r, w[:, :k].reshape(-1)[r] - 8:].any()
