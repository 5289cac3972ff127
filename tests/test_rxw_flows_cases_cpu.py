"""What the streams and call schedules of tests/test_gpu_rxw_flows.py contain, from the host objects (api.FecRxWindowHost) and
tools/rx_window_model.py alone: a GPU test that is green on inputs without these cases would show nothing about them."""
import numpy as np
import pytest

import rxw_cases as rc
import rxw_flows_cases as fc

wm = rc.wm
N = rc.N


def schedule_facts(nflows, W, A):
    streams = fc.lockstep_streams(nflows, A)
    facts = set()
    blocks_of = [[] for _ in range(nflows)]
    with fc.HostFlows(nflows, W, A) as hx:
        for call in fc.lockstep_calls(hx, streams, fc.lockstep_seed(nflows, W, A)):
            lens = [b - a for a, b in call.spans]
            _, fb = fc.concat(call.pieces)
            assert fb[-1] == sum(lens)
            unfinished = [a < streams[f].shape[0] for f, (a, _) in enumerate(call.spans)]
            if any(ln == 0 and u for ln, u in zip(lens, unfinished)):
                facts.add("empty segment of an unfinished flow")
            if any(ln == 0 for ln in lens) and sum(lens) > 0:
                facts.add("empty segment")
            stopped = [f for f in range(nflows) if call.closes[f] == call.mb and call.consumed[f] < lens[f]]
            whole = [f for f in range(nflows) if lens[f] > 0 and call.consumed[f] == lens[f]]
            if stopped and whole:
                facts.add("a flow stops at max_blocks while another consumes its segment")
            if any(int(b) % 64 for b in fb[1:-1]):
                facts.add("a segment begins off a multiple of 64")
            if any(call.closes[f] == 0 and lens[f] > 0 for f in range(nflows)) and call.closes.sum() > 0:
                facts.add("a flow closes nothing where others close")
            base = 0
            for f in range(nflows):
                blocks_of[f] += call.blocks[base:base + call.closes[f]].tolist()
                base += call.closes[f]
        stats = [hx.stats(f) for f in range(nflows)]
    for f in range(nflows):
        b = blocks_of[f]
        if any(x == 255 and y == 0 for x, y in zip(b[:-1], b[1:])):
            facts.add("a block number wraps through 255")
        by_ahead, resyncs = fc.count_ahead_closes(streams[f], W, A)
        assert resyncs == stats[f]["resyncs"], "the schedule's cuts do not change what the stream does"
        if by_ahead:
            facts.add("close by the ahead limit")
        if resyncs:
            facts.add("re-anchor")
    return facts


@pytest.mark.parametrize("W,A", fc.LOCKSTEP_WA)
@pytest.mark.parametrize("nflows", [n for n in fc.LOCKSTEP_NFLOWS if n > 1])
def test_lockstep_schedules_hold_their_cases(nflows, W, A):
    facts = schedule_facts(nflows, W, A)
    want = {"empty segment", "empty segment of an unfinished flow", "a flow stops at max_blocks while another consumes its segment",
            "a segment begins off a multiple of 64", "a flow closes nothing where others close", "a block number wraps through 255"}
    if A > 0:
        want |= {"close by the ahead limit", "re-anchor"}
    assert want <= facts, sorted(want - facts)


@pytest.mark.parametrize("W,A", fc.LOCKSTEP_WA)
def test_single_flow_schedule_wraps_and_stops(W, A):
    facts = schedule_facts(1, W, A)
    assert "a block number wraps through 255" in facts
    if A > 0:
        assert {"close by the ahead limit", "re-anchor"} <= facts


def test_streams_are_the_ones_named():
    for nflows in (3, 70):
        streams = fc.lockstep_streams(nflows, 10)
        assert len(streams) == nflows
        assert np.array_equal(streams[1], rc.random_stream(**rc.WRAP))
        assert np.array_equal(streams[-1], rc.packets_of(*rc.edge_stream(10)))
        assert np.array_equal(streams[0], rc.random_stream(rc.RANDOM_SEEDS[0]))
        blk, _ = wm.headers(streams[1])
        assert 255 in blk and 0 in blk


def test_host_flows_matches_the_model():
    """HostFlows's layout (dense in flow order) against tools/rx_window_model.py, flow by flow."""
    streams = fc.lockstep_streams(3, 10)
    with fc.HostFlows(3, 4, 10) as hx:
        closes, blocks, sym, er, consumed = hx.push_many(streams, 1 << 20)
        base = 0
        for f, pk in enumerate(streams):
            m = rc.model_run(pk, 4, 10)
            mb, ms, me = wm.planes(m.closed, pk, N)
            sl = slice(base, base + closes[f])
            assert consumed[f] == pk.shape[0] == m.consumed and closes[f] == len(m.closed)
            assert np.array_equal(blocks[sl], mb) and np.array_equal(sym[sl], ms) and np.array_equal(er[sl], me)
            assert hx.state(f) == m.state
            base += closes[f]
        assert base == len(blocks)


def test_flush_scenario_holds_its_cases():
    before, after = fc.flush_streams()
    assert fc.FLUSH_LIST != sorted(fc.FLUSH_LIST) and 3 not in fc.FLUSH_LIST and len(set(fc.FLUSH_LIST)) == len(fc.FLUSH_LIST)
    with fc.HostFlows(5, fc.FLUSH_W, fc.FLUSH_A) as hx:
        hx.push_many(before, 64)
        pend = hx.pending()
        assert hx.state(1)["base"] == -1 and pend[1] == 0, "flow 1 has nothing open"
        c2 = hx.state(2)["cnt"]
        assert c2[0] > 0 and c2[1] == 0 and c2[2] > 0 and pend[2] == 3, "flow 2: an empty slot between two non-empty ones"
        assert pend[3] >= 1 and pend[0] >= 1 and pend[4] >= 1
        closes, blocks, sym, er = hx.flush_many(fc.FLUSH_LIST)
        assert closes.tolist() == [pend[f] for f in fc.FLUSH_LIST] and len(blocks) == closes.sum()
        assert er[closes[0] + closes[1] + 1].all(), "the empty block between comes out all erased"
        assert hx.flush_many(fc.FLUSH_LIST)[0].sum() == 0
        assert hx.pending()[3] == pend[3], "the unlisted flow is untouched"
        c, b, *_ = hx.push_many(after, 64)
        assert c[3] >= 1 and c[1] >= 1, "flows go on after the flush"


def test_outage_stream_is_the_point():
    """The stream of the feature's test: the two-buffer rule closes 3 blocks, the window (W = 4, A = 10) 39."""
    blk, sym = rc.outage_stream()
    closed2, _ = wm.two_buffer(blk, sym, N, rc.K)
    r = wm.run(blk, sym, N, rc.K, 4, 10)
    assert len(closed2) < len(r.closed) and len(r.closed) >= 30
