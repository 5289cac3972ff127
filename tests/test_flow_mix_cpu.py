"""tools/flow_mix.py, the interleaver behind tests/test_gpu_flows_mixed.py, checked on the host alone: every pattern keeps each
flow's order (a stable sort by flow gives the segments and their flow_begin back), the patterns have the properties they are named
for, the numpy model of `left` is "rank >= used", and the `mixed` stream of tools/flow_streams.py contains a call in which a flow
stops at max_blocks_per_flow -- the only situation in which `left` is not all zero."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flow_mix as fm  # noqa: E402
import flow_streams as fs  # noqa: E402

TILE = 1024     # the partition's smallest tile (include/ldpc_erasure_amd_flows_mixed.h)


def segments_of(lens, plen=12, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(c, plen), dtype=np.uint8) for c in lens]


LENS = {"few": (0, 1, 7, 2500, 300), "wide": tuple([3] * 40 + [0, 5] * 20 + [70] * 10), "one": (0, 0, 1300, 0)}


@pytest.mark.parametrize("unrouted", [False, True])
@pytest.mark.parametrize("pattern", fm.PATTERNS)
@pytest.mark.parametrize("lens", sorted(LENS))
def test_stable_sort_gives_the_segments_back(lens, pattern, unrouted):
    segs = segments_of(LENS[lens])
    nf = len(segs)
    pk, flow_of = fm.mix(segs, pattern, 3, unrouted)
    assert flow_of.dtype == np.int32 and pk.shape == (flow_of.size, 12) and pk.flags["C_CONTIGUOUS"]
    routed = (flow_of >= 0) & (flow_of < nf)
    assert (routed.sum() < flow_of.size) == unrouted
    if unrouted:
        assert {-1, nf, 2**31 - 1} <= set(flow_of[~routed].tolist())
    # np.argsort(kind="stable") over the routed packets: the segments side by side, and their flow_begin
    idx = np.flatnonzero(routed)
    order = idx[np.argsort(flow_of[idx], kind="stable")]
    want, fb = fs.flow_begin_of(segs)
    assert np.array_equal(pk[order], want)
    assert np.array_equal(np.concatenate([[0], np.cumsum(np.bincount(flow_of[idx], minlength=nf))]), fb)
    o2, counts, fb2 = fm.demux(flow_of, nf)
    assert np.array_equal(o2, order) and np.array_equal(fb2, fb) and np.array_equal(counts, np.diff(fb))


def test_patterns_have_the_properties_they_are_named_for():
    rng = np.random.default_rng(1)
    # round robin: a group of 64 consecutive packets, starting at a multiple of 64, with 64 distinct flows
    ids = fm.flow_ids([5] * 70, "round_robin", rng)
    assert any(np.unique(ids[g:g + 64]).size == 64 for g in range(0, ids.size - 63, 64))
    assert np.array_equal(ids[:70], np.arange(70))
    # runs: a run of one flow longer than a wavefront and longer than a tile
    ids = fm.flow_ids([3000, 2500, 10], "runs", rng)
    edges = np.flatnonzero(np.diff(ids)) + 1
    runs = np.diff(np.concatenate([[0], edges, [ids.size]]))
    assert fm.RUN > TILE > 64 and runs.max() >= fm.RUN and (runs >= fm.RUN).sum() >= 4 and np.unique(ids[:3 * fm.RUN]).size == 3
    # single: one flow only
    assert (fm.flow_ids([0, 0, 77, 0], "single", rng) == 2).all()
    # reverse: the flows in descending order
    ids = fm.flow_ids([2, 0, 3, 1], "reverse", rng)
    assert ids.tolist() == [3, 2, 2, 2, 0, 0]
    # random: not sorted, and not the same for another seed
    a, b = fm.flow_of_for([100] * 8, "random", 1), fm.flow_of_for([100] * 8, "random", 2)
    assert (np.diff(a) < 0).any() and not np.array_equal(a, b) and np.array_equal(np.bincount(a), [100] * 8)
    # unrouted: all three kinds, also in an otherwise empty call
    assert set(fm.flow_of_for([0, 0], "random", 1, unrouted=True).tolist()) == {-1, 2, 2**31 - 1}


def test_left_model_is_rank_at_or_beyond_used():
    flow_of = fm.flow_of_for([5, 0, 9, 4], "random", 7, unrouted=True)
    used = np.array([5, 0, 3, 0])
    left = fm.left_model(flow_of, 4, used)
    rank = np.zeros(flow_of.size, dtype=np.int64)
    for p in range(flow_of.size):                       # the definition, packet by packet
        rank[p] = int((flow_of[:p] == flow_of[p]).sum())
    routed = (flow_of >= 0) & (flow_of < 4)
    want = np.array([1 if routed[p] and rank[p] >= used[flow_of[p]] else 0 for p in range(flow_of.size)], dtype=np.uint8)
    assert np.array_equal(left, want) and left.sum() == 6 + 4 and not left[~routed].any()


def test_mixed_stream_has_a_call_that_leaves_packets(oracle):
    from test_gpu_receiver import random_code
    code = random_code()
    sc = fs.scenario("mixed", oracle.OracleCode(code), code, 16)
    hits = 0
    for i, call in enumerate(sc["calls"]):
        offered = np.array([c["c"] for c in call["flows"]])
        used = np.array([c["used"] for c in call["flows"]])
        closes = np.array([len(c["blocks"]) for c in call["flows"]])
        stopped = (used < offered)
        assert (closes[stopped] == call["mb"]).all()        # the only reason to leave packets
        if stopped.any() and (~stopped & (offered > 0)).any():
            segs = [sc["flows"][f][c["pos"]:c["pos"] + c["c"]] for f, c in enumerate(call["flows"])]
            pk, flow_of = fm.mix(segs, fm.PATTERNS[i % len(fm.PATTERNS)], i, unrouted=True)
            left = fm.left_model(flow_of, len(segs), used)
            assert left.sum() == (offered - used).sum() > 0
            for f in np.flatnonzero(stopped):               # what is left of a flow is the tail of its segment
                assert np.array_equal(pk[(flow_of == f) & (left == 1)], segs[f][used[f]:])
            hits += 1
    assert hits >= 1
