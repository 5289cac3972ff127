"""CPU test of the multi-flow interleaved order (ldpc_amd_fec_tx_flows_ilv_layout, include/ldpc_erasure_amd_interleave_flows.h)
against the brute-force multiplexer of tools/interleave_model.py (flows_order): every flow's substream from the single-flow model,
merged packet by packet.  The library computes the same positions in closed form (a first packet and a stride per frame); the
multiplexer knows nothing of that form."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ldpc_erasure_codes_amd import api

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import interleave_model as im  # noqa: E402

EINVAL = -1
SEG, RR = api.TX_SEGMENTED, api.TX_ROUND_ROBIN
assert (SEG, RR) == (im.SEGMENTED, im.ROUND_ROBIN)
DEPTHS = api.ILV_DEPTHS


def positions(first, stride, n):
    return first[:, None] + np.arange(n, dtype=np.int64)[None, :] * stride[:, None].astype(np.int64)


def check(counts, n, block0, D, order):
    """The library's layout against the multiplexer: the wire position of every (frame, row), a permutation of 0 .. F n - 1."""
    fb = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    F = int(fb[-1])
    first, stride = api.fec_tx_flows_ilv_layout(fb, n, block0, D, order)
    assert first.dtype == np.int64 and stride.dtype == np.int32 and first.shape == stride.shape == (F,)
    got = positions(first, stride, n)
    frame, row, flow = im.flows_order(fb, n, block0, D, order)
    assert frame.shape == (F * n,)
    want = np.full((F, n), -1, dtype=np.int64)
    want[frame, row] = np.arange(F * n)
    assert np.array_equal(got, want), (counts, n, block0, D, order)
    assert np.array_equal(np.sort(got.ravel()), np.arange(F * n)), "not a permutation"
    assert np.array_equal(flow, np.searchsorted(fb, frame, side="right") - 1)
    return first, stride


def group_counts(nflows, D, seed, top):
    """Unequal multiples of D, zeros among them (with more than one flow)."""
    c = np.random.default_rng(seed).integers(0, top + 1, size=nflows) * D
    if nflows > 1:
        c[nflows // 2], c[0], c[nflows - 1] = 0, top * D, D
    else:
        c[0] = max(int(c[0]), D)
    return c


def wrap_block0(nflows, D, seed, aligned):
    """Block numbers whose frames cross the 8-bit wrap for some flows; multiples of D where the order needs them."""
    b = (256 - np.random.default_rng(seed).integers(0, 3 * D + 2, size=nflows)) & 0xFF
    return (b // D * D) & 0xFF if aligned else b


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("nflows", [1, 3, 70])
@pytest.mark.parametrize("n", [7, 200])
def test_round_robin_is_the_multiplexed_substreams(n, nflows, D):
    top = 3 if n == 7 else 2
    counts = group_counts(nflows, D, 10 * D + nflows, top)
    block0 = wrap_block0(nflows, D, 20 * D + nflows, aligned=True)
    block0[0] = 256 - D   # flow 0, the longest: its second group starts at block 0
    assert nflows == 1 or ((counts == 0).any() and len(set(counts.tolist())) > 2), "an empty flow and unequal counts"
    first, stride = check(counts, n, block0, D, RR)
    if D > 1:   # the closed form's stride: D times the flows active in the frame's group
        fb = np.concatenate([[0], np.cumsum(counts)])
        for f in range(nflows):
            for i in range(int(counts[f])):
                assert stride[fb[f] + i] == D * int((counts > i // D * D).sum())


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("nflows", [1, 3, 70])
@pytest.mark.parametrize("n", [7, 200])
def test_segmented_is_the_shifted_single_flow_layouts(n, nflows, D):
    """Any counts and block numbers: short first and last runs included."""
    rng = np.random.default_rng(30 * D + nflows + n)
    counts = rng.integers(0, 2 * D + 3, size=nflows)
    counts[0] = 2 * D
    block0 = wrap_block0(nflows, D, 40 * D + nflows, aligned=False)
    block0[0] = (256 - D - 1) & 0xFF   # a first run of one frame where D > 1, then a whole one across the wrap, then a short last one
    first, stride = check(counts, n, block0, D, SEG)
    fb = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    for f in range(nflows):
        f1, s1 = api.fec_tx_ilv_layout(int(counts[f]), n, int(block0[f]), D)
        assert np.array_equal(first[fb[f]:fb[f + 1]], f1 + n * fb[f]) and np.array_equal(stride[fb[f]:fb[f + 1]], s1), f
    if D > 1:
        assert stride[0] == 1 and stride[1] == D and stride[fb[1] - 1] < D, "short first and last runs"


def test_depth_1_is_the_multi_flow_layout():
    rng = np.random.default_rng(5)
    for _ in range(100):
        nflows = int(rng.integers(1, 10))
        n = int(rng.integers(1, 8))
        fb = np.concatenate([[0], np.cumsum(rng.integers(0, 6, size=nflows))]).astype(np.int64)
        block0 = rng.integers(0, 256, size=nflows)
        for order in (SEG, RR):
            a, b = api.fec_tx_flows_ilv_layout(fb, n, block0, 1, order), api.fec_tx_flows_layout(fb, n, order)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            check(np.diff(fb), n, block0, 1, order)


def test_one_flow_is_the_single_flow_layout_in_both_orders():
    for D in DEPTHS:
        for order in (SEG, RR):
            a = api.fec_tx_flows_ilv_layout([0, 3 * D], 7, 256 - D, D, order)
            b = api.fec_tx_ilv_layout(3 * D, 7, 256 - D, D)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_layout_refusals_need_no_device():
    L = api.load_library()

    def call(nflows, fb, n, block0, depth, order, want_out=True):
        fb = None if fb is None else np.ascontiguousarray(fb, dtype=np.int64)
        b0 = None if block0 is None else np.ascontiguousarray(block0, dtype=np.uint8)
        F = 0 if fb is None else max(int(fb[-1]), 0)
        first, stride = np.full(max(F, 1), -5, dtype=np.int64), np.full(max(F, 1), -5, dtype=np.int32)
        rc = L.ldpc_amd_fec_tx_flows_ilv_layout(nflows, None if fb is None else fb.ctypes.data, n, None if b0 is None else b0.ctypes.data, depth, order,
                                                first.ctypes.data if want_out else None, stride.ctypes.data if want_out else None)
        if rc < 0:
            assert (first == -5).all() and (stride == -5).all(), "a refused call writes nothing"
        return rc

    assert call(2, [0, 4, 12], 5, [4, 252], 4, RR) == 60                       # (a good call, for contrast)
    assert call(2, [0, 4, 12], 5, [4, 252], 4, RR, want_out=False) == 60       # first / stride may be NULL
    assert call(3, [0, 4, 4, 12], 5, [4, 3, 252], 4, RR) == 60                 # an empty flow is fine, whatever its block0
    for depth in (0, 3, 5, 32, -1):
        assert call(2, [0, 4, 12], 5, [4, 252], depth, RR) == EINVAL           # a depth outside the set
        assert call(2, [0, 4, 12], 5, [4, 252], depth, SEG) == EINVAL
    assert call(2, [0, 4, 12], 5, None, 4, RR) == EINVAL                       # block0 NULL
    assert call(2, [0, 4, 12], 5, [4, 250], 4, RR) == EINVAL                   # part groups: block0 off a multiple of the depth
    assert call(2, [0, 4, 11], 5, [4, 252], 4, RR) == EINVAL                   # part groups: a count that is no multiple
    assert call(2, [0, 4, 11], 5, [5, 250], 4, SEG) == 55                      # SEGMENTED has no such condition
    assert call(2, [0, 4, 11], 5, [5, 250], 1, RR) == 55                       # nor has depth 1
    assert call(0, [0], 4, [0], 2, RR) == EINVAL                               # the refusals of ldpc_amd_fec_tx_flows_layout
    assert call(4097, np.arange(4098) * 2, 4, [0] * 4097, 2, RR, want_out=False) == EINVAL
    assert call(2, None, 4, [0, 0], 2, RR) == EINVAL
    assert call(2, [2, 4, 6], 4, [0, 0], 2, RR) == EINVAL
    assert call(2, [0, 4, 2], 4, [0, 0], 2, SEG) == EINVAL
    assert call(2, [0, 2, 4], 0, [0, 0], 2, RR) == EINVAL
    assert call(2, [0, 2, 4], 4, [0, 0], 2, 2) == EINVAL
    assert call(1, [0, 1 << 20], 2048, [0], 2, RR, want_out=False) == EINVAL   # F * n >= 2^31
    assert call(1, [0, 1 << 20], 2048, [0], 2, SEG, want_out=False) == EINVAL
    assert call(1, [0, (1 << 20) - 2], 2048, [0], 2, SEG, want_out=False) == ((1 << 20) - 2) * 2048
    with pytest.raises(api.LdpcAmdError):
        api.fec_tx_flows_ilv_layout([0, 4, 12], 5, [4, 250], 4, RR)
    with pytest.raises(api.LdpcAmdError):
        api.fec_tx_flows_ilv_layout([0, 4, 12], 5, 0, 3, SEG)
