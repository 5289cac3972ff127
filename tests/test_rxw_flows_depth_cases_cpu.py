"""What the streams of tests/test_gpu_rxw_flows_depth.py contain, from tools/rx_window_model.py and the host objects
(api.FecRxWindowHost(depth = D)) alone: a GPU test that is green on inputs without these cases would show nothing about them.  In
particular every stream is one on which the plain rule (D = 1) and the depth-D rule differ, so a multi-flow receiver that ignored
its depth would fail the lockstep test."""
import numpy as np
import pytest

import interleave_cases as ic
import rxw_cases as rc
import rxw_flows_cases as fc
import rxw_flows_depth_cases as dc

wm = rc.wm
N = rc.N


@pytest.mark.parametrize("A", dc.AHEAD)
@pytest.mark.parametrize("W,D", dc.LOCKSTEP_WD)
@pytest.mark.parametrize("nflows", dc.LOCKSTEP_NFLOWS)
def test_lockstep_streams_hold_their_cases(nflows, W, D, A):
    """Every lockstep configuration has a flow with a g == 1 close and -- where there is an ahead limit: nothing else forces a close
    or re-anchors -- one with a forced close and one with a re-anchor below the first block seen; on every stream the plain rule
    gives other closes or another late count."""
    streams = dc.lockstep_streams(nflows, W, D, A)
    assert len(streams) == nflows
    facts = [dc.stream_facts(pk, W, A, D) for pk in streams]
    want = dc.WANT if A > 0 else {"g == 1 close"}
    have = set().union(*facts)
    assert want <= have, sorted(want - have)
    for f, (pk, fa) in enumerate(zip(streams, facts)):
        assert pk.shape[0] == 0 or "the plain rule differs" in fa, f
    e = dc.empty_flow(nflows)
    assert (e is None) == (nflows <= 2) and (e is None or streams[e].shape[0] == 0), "one flow gets nothing"


def test_streams_are_the_ones_named():
    for nflows in (3, 70):
        for W, D in dc.LOCKSTEP_WD:
            streams = dc.lockstep_streams(nflows, W, D, 10)
            assert np.array_equal(streams[0], ic.stream(7001 + 100 * D, D, 248, 0))
            if nflows == 70:
                assert np.array_equal(streams[2], ic.stream(7001 + 100 * D + 2, D, 248, 64))
                assert np.array_equal(streams[3], ic.stream(7001 + 100 * D + 3, D, 250, 64))
                assert np.array_equal(streams[5], ic.stream(7001 + 100 * D + 5, D, 250, 0))
                seeds = [dc.stream_args(f, D)[0] for f in range(nflows)]
                assert len(set(seeds)) == nflows and sum(s != 7001 + 100 * D + f for f, s in enumerate(seeds)) <= 5, "a different seed per flow"
            edge = (W, D) == (32, 16)
            assert np.array_equal(streams[-1], rc.packets_of(*ic.edge_stream())) == edge
    assert np.array_equal(dc.lockstep_streams(1, 32, 16, 0)[0], rc.packets_of(*ic.edge_stream()))
    assert np.array_equal(dc.lockstep_streams(1, 32, 16, 10)[0], ic.stream(7001 + 1600, 16, 248, 0))
    assert ic.edge_facts(ic.edge_calls()) >= {"g == 1 close and re-anchor in a group", "re-anchor into a slot above 0"}
    blk, _ = wm.headers(rc.packets_of(*ic.edge_stream()))
    assert 255 in blk and 0 in blk and 69 in blk


@pytest.mark.parametrize("W,D", dc.LOCKSTEP_WD)
def test_host_flows_depth_matches_the_model(W, D):
    """HostFlowsDepth's layout (dense in flow order) against tools/rx_window_model.py at depth D, flow by flow, and its flush."""
    streams = dc.lockstep_streams(3, W, D, 10)
    with dc.HostFlowsDepth(3, W, 10, D) as hx:
        closes, blocks, sym, er, consumed = hx.push_many(streams, 1 << 20)
        base = 0
        models = []
        for f, pk in enumerate(streams):
            w = wm.Window(N, rc.K, W, 10, D)
            closed, used = w.push_many(*wm.headers(pk), 1 << 30)
            mb, ms, me = wm.planes(closed, pk, N)
            sl = slice(base, base + closes[f])
            assert consumed[f] == pk.shape[0] == used and closes[f] == len(closed)
            assert np.array_equal(blocks[sl], mb) and np.array_equal(sym[sl], ms) and np.array_equal(er[sl], me)
            if pk.shape[0]:
                assert hx.state(f) == w.state() and hx.stats(f) == w.totals
            base += closes[f]
            models.append((w, pk))
        assert base == len(blocks)
        assert hx.pending() == [max([d + 1 for d, c in enumerate(w.cnt) if c > 0], default=0) for w, _ in models]
        fcl, fbl, fsym, fer = hx.flush_many([2, 0])
        want = [wm.planes(models[f][0].flush(), models[f][1], N) for f in (2, 0)]
        assert fcl.tolist() == [len(w[0]) for w in want] and np.array_equal(fbl, np.concatenate([w[0] for w in want]))
        assert np.array_equal(fsym, np.concatenate([w[1] for w in want])) and np.array_equal(fer, np.concatenate([w[2] for w in want]))


def test_lockstep_schedule_cuts_the_streams():
    """The schedule of tests/rxw_flows_cases.py on these streams: many calls, flows that stop at max_blocks_per_flow, empty segments."""
    nflows, (W, D), A = 3, dc.LOCKSTEP_WD[1], 10
    streams = dc.lockstep_streams(nflows, W, D, A)
    ncalls = stopped = empty = 0
    with dc.HostFlowsDepth(nflows, W, A, D) as hx:
        for call in fc.lockstep_calls(hx, streams, dc.lockstep_seed(nflows, W, A, D)):
            lens = [b - a for a, b in call.spans]
            stopped += any(call.closes[f] == call.mb and call.consumed[f] < lens[f] for f in range(nflows))
            empty += any(ln == 0 for ln in lens) and sum(lens) > 0
            ncalls += 1
    assert ncalls >= 8 and stopped >= 1 and empty >= 1
