"""CPU test of the multi-flow sender's order (ldpc_amd_fec_tx_flows_layout, include/ldpc_erasure_amd_sender_flows.h) against a
LITERAL simulation of the multiplexer written here: round after round, every flow that still has a packet emits its next one,
flows in ascending order.  The library computes the same positions in closed form (a first packet and a stride per frame); the
simulation knows nothing of that form."""
import ctypes as C

import numpy as np
import pytest

from ldpc_erasure_codes_amd import api

EINVAL = -1
SEG, RR = api.TX_SEGMENTED, api.TX_ROUND_ROBIN


def simulate_round_robin(counts, n):
    """pos[t][j] = wire index of row j of frame t (frames of all flows side by side, flow after flow), by playing the rounds."""
    counts = [int(c) for c in counts]
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pos = np.full((int(begin[-1]), n), -1, dtype=np.int64)
    sent = [0] * len(counts)          # packets each flow has emitted
    p = 0
    while any(sent[f] < counts[f] * n for f in range(len(counts))):
        for f in range(len(counts)):  # one round
            q = sent[f]
            if q < counts[f] * n:
                pos[begin[f] + q // n, q % n] = p
                p += 1
                sent[f] += 1
    return begin, pos


def simulate_segmented(counts, n):
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    F = int(begin[-1])
    return begin, np.arange(F * n, dtype=np.int64).reshape(F, n)


def library_positions(begin, n, order):
    first, stride = api.fec_tx_flows_layout(begin, n, order)
    assert first.dtype == np.int64 and stride.dtype == np.int32 and first.shape == stride.shape == (int(begin[-1]),)
    return first[:, None] + np.arange(n, dtype=np.int64)[None, :] * stride[:, None].astype(np.int64)


def check(counts, n):
    begin, want = simulate_round_robin(counts, n)
    got = library_positions(begin, n, RR)
    assert np.array_equal(got, want), (counts, n)
    P = int(begin[-1]) * n
    assert np.array_equal(np.sort(got.ravel()), np.arange(P)), "not a permutation"
    seg = library_positions(begin, n, SEG)
    assert np.array_equal(seg.ravel(), np.arange(P)), "SEGMENTED is not the identity"
    assert np.array_equal(seg, simulate_segmented(counts, n)[1])


def test_random_flow_shapes_match_the_simulated_rounds():
    rng = np.random.default_rng(20240607)
    for _ in range(300):
        nflows = int(rng.integers(1, 10))
        n = int(rng.integers(1, 8))
        check(rng.integers(0, 6, size=nflows), n)


@pytest.mark.parametrize("counts,n", [
    ((0, 0, 0), 3),            # all flows empty
    ((0,), 4),
    ((5,), 7),                 # a single flow: the single-flow order
    ((1,), 1),
    ((3,) * 8, 5),             # all flows equal: stride nflows throughout
    ((2, 0, 5), 6),            # unequal, an empty flow, the stride changes mid-stream
    ((0, 4, 0, 1, 0), 2),
    ((5, 4, 3, 2, 1, 0), 3),
])
def test_named_flow_shapes(counts, n):
    check(counts, n)


def test_4096_flows_of_one_frame():
    n = 3
    check((1,) * 4096, n)
    first, stride = api.fec_tx_flows_layout(np.arange(4097), n, RR)
    assert np.array_equal(first, np.arange(4096)) and (stride == 4096).all()


def test_single_flow_round_robin_is_segmented():
    fb = np.array([0, 9])
    for n in (1, 4):
        a, b = api.fec_tx_flows_layout(fb, n, RR), api.fec_tx_flows_layout(fb, n, SEG)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[1] == 1).all()


def test_layout_refusals_need_no_device():
    L = api.load_library()

    def call(nflows, fb, n, order, want_out=True):
        fb = None if fb is None else np.ascontiguousarray(fb, dtype=np.int64)
        F = 0 if fb is None else max(int(fb[-1]), 0)
        first, stride = np.zeros(max(F, 1), dtype=np.int64), np.zeros(max(F, 1), dtype=np.int32)
        return L.ldpc_amd_fec_tx_flows_layout(nflows, None if fb is None else fb.ctypes.data, n, order,
                                              first.ctypes.data if want_out else None, stride.ctypes.data if want_out else None)

    assert call(2, [0, 1, 3], 4, RR) == 12                                  # (a good call, for contrast)
    assert call(2, [0, 1, 3], 4, RR, want_out=False) == 12                  # first / stride may be NULL
    assert call(0, [0], 4, RR) == EINVAL                                    # nflows outside 1..4096
    assert call(-1, [0], 4, RR) == EINVAL
    assert call(4097, np.arange(4098), 4, RR, want_out=False) == EINVAL
    assert call(4096, np.arange(4097), 4, RR) == 4096 * 4
    assert call(2, None, 4, RR) == EINVAL                                   # frame_begin NULL
    assert call(2, [1, 2, 3], 4, RR) == EINVAL                              # does not start at 0
    assert call(2, [0, 3, 2], 4, RR) == EINVAL                              # decreases
    assert call(2, [0, 1, 3], 0, RR) == EINVAL                              # n < 1
    assert call(2, [0, 1, 3], 4, 2) == EINVAL                               # unknown order
    assert call(2, [0, 1, 3], 4, -1) == EINVAL
    # F * n >= 2^31: refused before anything is written (the arrays above hold one entry)
    assert call(1, [0, 1 << 20], 2048, RR, want_out=False) == EINVAL
    assert call(1, [0, 1 << 20], 2048, SEG, want_out=False) == EINVAL
    assert call(1, [0, (1 << 20) - 1], 2048, SEG, want_out=False) == ((1 << 20) - 1) * 2048
    with pytest.raises(api.LdpcAmdError):
        api.fec_tx_flows_layout([0, 2, 1], 3, RR)
    with pytest.raises(api.LdpcAmdError):
        api.fec_tx_flows_layout([0, 2], 3, 7)
