"""What the interleaved calls of tests/test_gpu_rxw_flows_mixed.py contain, from the host objects (api.FecRxWindowHost) and
tools/flow_mix.py alone: de-interleaving every mixed call gives the segmented call back, and every lockstep configuration holds a
call in which a flow stops short (so `left` has ones), a call with an empty flow and a call of more than one partition tile."""
import numpy as np
import pytest

import rxw_flows_cases as fc
import rxw_flows_mixed_cases as mc

fm = mc.fm
TILE = 1024   # the partition's smallest tile, in packets


@pytest.mark.parametrize("W,A", fc.LOCKSTEP_WA)
@pytest.mark.parametrize("nflows", fc.LOCKSTEP_NFLOWS)
def test_mixed_lockstep_calls_hold_their_cases(nflows, W, A):
    streams = fc.lockstep_streams(nflows, A)
    seed = fc.lockstep_seed(nflows, W, A)
    stopping = empty = longest = unrouted = 0
    patterns = set()
    with fc.HostFlows(nflows, W, A) as hx:
        for i, call in enumerate(fc.lockstep_calls(hx, streams, seed)):
            pk, flow_of = mc.mixed_call(call, i, seed)
            lens = np.array([p.shape[0] for p in call.pieces], dtype=np.int64)
            want_pk, want_fb = fc.concat(call.pieces)
            got_pk, got_fb = mc.deinterleave(pk, flow_of, nflows)
            assert np.array_equal(got_fb, want_fb) and np.array_equal(np.diff(got_fb), lens), i
            assert np.array_equal(got_pk, want_pk), i
            assert pk.shape[0] == flow_of.size == lens.sum() + mc.unrouted_in(flow_of, nflows)
            left = fm.left_model(flow_of, nflows, call.consumed)
            assert left.sum() == (lens - call.consumed).sum()
            stopping += int((call.consumed < lens).any() and left.any())
            empty += int((lens == 0).any())
            longest = max(longest, int(flow_of.size))
            unrouted += mc.unrouted_in(flow_of, nflows)
            patterns.add(fm.PATTERNS[i % len(fm.PATTERNS)])
    assert stopping >= 1, "a call in which some flow stops short of what it was offered"
    assert empty >= 1, "a call with an empty flow"
    assert longest > TILE, "a call of two or more partition tiles"
    assert unrouted > 0 and patterns == set(fm.PATTERNS)


def test_short_calls_take_short_runs():
    """The `runs` pattern alternates flows inside a short call too: with the default run a call below 1100 packets per flow would be
    the `single` pattern."""
    rng = np.random.default_rng(3)
    pieces = [rng.integers(0, 256, size=(c, 8 + fc.S), dtype=np.uint8) for c in (200, 150, 0, 90)]
    call = fc.Call(1, None, pieces, None, None, None, None, None)
    _, flow_of = mc.mixed_call(call, 2, 5)   # call 2: "runs", no unrouted packets
    assert fm.PATTERNS[2] == "runs" and flow_of.size == 440
    changes = int((np.diff(flow_of) != 0).sum())
    assert changes > 3, "more flow changes than flow by flow"
    assert flow_of[:mc.SHORT_RUN].tolist() == [0] * mc.SHORT_RUN
