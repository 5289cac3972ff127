"""The windowed receiver's rule without a GPU (include/ldpc_erasure_amd_rx_window.h): the C host object (csrc/rx_window.cpp) against
the numpy model (tools/rx_window_model.py), the W = 2, A = 0 anchor against the two-buffer receiver, what the rule buys on an outage
and on a delay spread, call splitting, and flush.  Streams: tests/rxw_cases.py."""
import numpy as np
import pytest

import rxw_cases as rc
from ldpc_erasure_codes_amd import api

wm = rc.wm
N, K, S = rc.N, rc.K, rc.S

_STREAMS = {}


def stream(seed):
    if seed not in _STREAMS:
        _STREAMS[seed] = rc.random_stream(**rc.WRAP) if seed == "wrap" else rc.random_stream(seed)
    return _STREAMS[seed]


SEEDS = rc.RANDOM_SEEDS + ["wrap"]


def assert_equals_model(h, m, pk):
    mb, ms, me = wm.planes(m.closed, pk, N)
    assert h["blocks"] == mb.tolist()
    assert np.array_equal(h["sym"], ms) and np.array_equal(h["er"], me)
    assert h["stats"] == m.totals and h["state"] == m.state
    assert h["dropped"] == m.totals["bad_symbol"] + m.totals["late"] + m.totals["ahead_total"]
    assert sum(h["used"]) == m.consumed == pk.shape[0]


@pytest.mark.parametrize("seed", SEEDS)
def test_host_equals_model_on_random_streams(seed):
    pk = stream(seed)
    for W, A in rc.WA:
        assert_equals_model(rc.host_run(pk, W, A), rc.model_run(pk, W, A), pk)


def test_streams_exercise_the_rule():
    """What the random streams contain, asserted on the model alone: duplicates, foreign and bad headers, a block number that wraps,
    closes by the count rule and by the ahead limit, re-anchors, and packets of all four classes."""
    resyncs = trips = 0
    for seed in SEEDS:
        pk = stream(seed)
        blk, sym = wm.headers(pk)
        assert (sym >= N).any() and np.unique(blk).size > 14
        assert np.unique(np.stack([blk, sym]), axis=1).shape[1] < pk.shape[0], "duplicates"
        for W, A in rc.WA[1:]:
            m = rc.model_run(pk, W, A)
            resyncs += m.totals["resyncs"]
            trips += m.totals["ahead_total"] > A
            assert m.totals["bad_symbol"] > 0 and m.totals["closed"] > 0
    assert resyncs >= 5 and trips >= 20
    blk, _ = wm.headers(stream("wrap"))
    m = rc.model_run(stream("wrap"), 4, 10)
    got = [b for b, _ in m.closed]
    assert 255 in got and 0 in got and got.index(0) == got.index(255) + 1, "the window moves across the wrap of the block number"


@pytest.mark.parametrize("seed", SEEDS[::3])
def test_host_equals_model_packet_by_packet(seed):
    pk = stream(seed)
    blk, sym = wm.headers(pk)
    for W, A in rc.WA[1::2]:
        w = wm.Window(N, K, W, A)
        with api.FecRxWindowHost(N, K, S, W, A) as rx:
            for p in range(pk.shape[0]):
                r, h = w.push(int(blk[p]), int(sym[p])), rx.push(pk[p])
                assert (r is None) == (h is None), (p, W, A)
                if r is not None:
                    _, ms, me = wm.planes([r], pk, N)
                    assert h[0] == r[0] and np.array_equal(h[1], ms[0]) and np.array_equal(h[2], me[0]), (p, W, A)
                if p % 97 == 0 or r is not None:
                    assert rx.state() == w.state() and rx.stats() == w.totals, (p, W, A)


@pytest.mark.parametrize("seed", SEEDS)
def test_anchor_window_2_ahead_0_is_the_two_buffer_receiver(seed):
    pk = stream(seed)
    for mb in (1, 3, 1 << 10):
        old, new = api.FecRx(N, K, S), api.FecRxWindowHost(N, K, S, 2, 0)
        pos = 0
        while pos < pk.shape[0]:
            a, b = old.push_many(pk[pos:], mb), new.push_many(pk[pos:], mb)
            assert a[3] == b[3] and a[3] > 0 and np.array_equal(a[0], b[0])
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            assert old.dropped == new.dropped
            pos += a[3]
        st = new.stats()
        assert st["ahead_total"] == 0 and st["resyncs"] == 0 and new.dropped == st["bad_symbol"] + st["late"]
        old.close()
        new.close()
    blk, sym = wm.headers(pk)
    closed, dropped = wm.two_buffer(blk, sym, N, K)
    m = rc.model_run(pk, 2, 0)
    assert closed == m.closed and dropped == m.totals["bad_symbol"] + m.totals["late"]


def test_outage_one_block_at_half():
    """40 blocks, 95 % kept, block 3 at 50 %: the two-buffer receiver stalls behind block 3, the windowed one loses that block and
    A + 1 packets."""
    blk, sym = rc.outage_stream()
    pk = rc.packets_of(blk, sym)
    old = api.FecRx(N, K, S)
    closed_old = len(old.push_many(pk, 64)[0])
    old.close()
    assert closed_old < 5
    assert closed_old == len(wm.two_buffer(blk, sym, N, K)[0])
    for W in (2, 4):
        A = 10
        h = rc.host_run(pk, W, A)
        assert_equals_model(h, rc.model_run(pk, W, A), pk)
        assert len(h["blocks"]) >= 38
        rows = N - h["er"].sum(axis=1)
        assert all(r >= K for b, r in zip(h["blocks"], rows) if b != 3) and 3 in h["blocks"]
        assert h["stats"]["ahead_total"] <= 2 * (A + 1) and h["stats"]["resyncs"] == 0


def test_outage_eighteen_blocks_lost():
    """Blocks 3 .. 20 missing: one re-anchor, and every block from 22 on closes (the last one, 39, is open with more than k
    packets when the stream ends)."""
    blk, sym = rc.long_outage_stream()
    pk = rc.packets_of(blk, sym)
    for W in (2, 4):
        h = rc.host_run(pk, W, 10)
        assert_equals_model(h, rc.model_run(pk, W, 10), pk)
        assert h["stats"]["resyncs"] == 1
        assert [b for b in h["blocks"] if b >= 22] == list(range(22, 39)) and h["state"]["base"] == 39 and h["state"]["cnt"][0] > K
        rows = N - h["er"].sum(axis=1)
        assert all(r >= K for b, r in zip(h["blocks"], rows) if b >= 22)
    old = api.FecRx(N, K, S)
    assert len(old.push_many(pk, 64)[0]) < 5
    old.close()


def test_reordering_over_five_blocks():
    """60 blocks, 90 % kept, delays uniform in 0 .. 1000 packet times: W = 8 closes at least 58 blocks, all with at least k rows;
    W = 2 hands out almost none with k rows."""
    pk = rc.reordered_stream()
    good = {}
    for W in (2, 8):
        h = rc.host_run(pk, W, 10)
        assert_equals_model(h, rc.model_run(pk, W, 10), pk)
        rows = N - h["er"].sum(axis=1)
        good[W] = (len(h["blocks"]), int((rows >= K).sum()))
    assert good[8][0] >= 58 and good[8][1] == good[8][0]
    assert not (good[2][0] >= 58 and good[2][1] == good[2][0]) and good[2][1] < 5


def event_cuts(pk, W, A):
    blk, sym = wm.headers(pk)
    ev = wm.events(blk, sym, N, K, W, A)
    return ev, sorted({p + 1 + o for p, _ in ev for o in (-2, -1, 0, 1, 2) if 0 < p + 1 + o < pk.shape[0]})


@pytest.mark.parametrize("seed", [SEEDS[1], SEEDS[6], "wrap"])
def test_splitting_a_stream_at_every_event(seed):
    """Two push_many calls, split within +-2 packets of every close and re-anchor, and calls that stop at max_blocks: what one call gives."""
    pk = stream(seed)
    kinds = set()
    for W, A in [(2, 10), (4, 10), (16, 3)]:
        one = rc.host_run(pk, W, A)
        ev, cuts = event_cuts(pk, W, A)
        kinds |= {k for _, k in ev}
        assert len(ev) >= 3
        for c in cuts:
            two = rc.host_run(pk, W, A, cuts=(c,))
            assert two["used"] == [c, pk.shape[0] - c]
            for key in ("blocks", "stats", "state", "dropped"):
                assert two[key] == one[key], (W, A, c, key)
            assert np.array_equal(two["sym"], one["sym"]) and np.array_equal(two["er"], one["er"]), (W, A, c)
        for mb in (1, 2):   # every call but the last stops at the packet that closed its max_blocks-th block
            parts = rc.host_run(pk, W, A, max_blocks=mb)
            closes = [p + 1 for p, k in ev if k == "close"]
            assert np.cumsum(parts["used"]).tolist()[:-1] == closes[mb - 1::mb][:len(parts["used"]) - 1]
            assert parts["blocks"] == one["blocks"] and parts["stats"] == one["stats"] and parts["state"] == one["state"]
            assert np.array_equal(parts["sym"], one["sym"]) and np.array_equal(parts["er"], one["er"])
    assert kinds == ({"close"} if seed == SEEDS[6] else {"close", "resync"})


def test_flush_hands_out_the_window_with_its_gaps():
    blk = np.array([7, 7, 9, 9, 9, 7], dtype=np.int64)
    sym = np.array([0, 5, 1, 2, 2, 199], dtype=np.int64)
    pk = rc.packets_of(blk, sym, seed=3)
    with api.FecRxWindowHost(N, K, S, 4, 10) as rx:
        assert len(rx.flush()[0]) == 0 and rx.state()["base"] == -1
        assert len(rx.push_many(pk, 4)[0]) == 0 and rx.state() == {"base": 7, "cnt": [3, 0, 3, 0], "ahead": 0}
        blocks, sy, er = rx.flush()
        assert blocks.tolist() == [7, 8, 9]
        w = wm.Window(N, K, 4, 10)
        w.push_many(blk, sym, 4)
        mb, ms, me = wm.planes(w.flush(), pk, N)
        assert np.array_equal(sy, ms) and np.array_equal(er, me) and mb.tolist() == [7, 8, 9]
        assert er[1].all() and not sy[1].any(), "the empty block between two non-empty ones is all erased"
        assert np.flatnonzero(er[0] == 0).tolist() == [0, 5, 199] and np.array_equal(sy[2, 2], pk[4, 8:]), "the last copy wins"
        assert rx.state() == {"base": 10, "cnt": [0, 0, 0, 0], "ahead": 0} == w.state() and rx.stats()["closed"] == 3
        assert len(rx.flush()[0]) == 0
        # the planes were reset: block 10 arrives into a clean slot
        assert len(rx.push_many(rc.packets_of([10], [4]), 1)[0]) == 0
        blocks, sy, er = rx.flush()
        assert blocks.tolist() == [10] and np.flatnonzero(er[0] == 0).tolist() == [4]


@pytest.mark.parametrize("A", rc.EDGE_A)
@pytest.mark.parametrize("W", rc.EDGE_W)
def test_plan_edge_stream_places_its_events(W, A):
    """The stream and the call boundaries of the GPU plan-edge test do what that test is for -- on the model alone -- and the host
    object agrees with the model on them."""
    blk, sym = rc.edge_stream(A)
    calls = rc.edge_calls(blk, sym, W, A)
    facts = rc.edge_facts(blk, sym, W, A, calls)
    want = {"lane0", "lane63", "last packet of a call", "two closes in a group", "short call"}
    if A > 0:
        want.add("close and re-anchor in a group")
    assert want <= facts, want - facts
    m = wm.run(blk, sym, N, K, W, A)
    got = [b for b, _ in m.closed]
    assert got[:7] == [250, 251, 252, 253, 254, 255, 0] and m.totals["resyncs"] == (1 if A > 0 else 0)
    assert m.totals["bad_symbol"] == 1 and m.totals["late"] >= 1
    pk = rc.packets_of(blk, sym)
    h = rc.host_run(pk, W, A, cuts=[s for s, _ in calls])
    assert_equals_model(h, m, pk)


def test_create_refuses_bad_parameters():
    for W, A in [(1, 0), (33, 0), (0, 5), (4, -1)]:
        with pytest.raises(api.LdpcAmdError):
            api.FecRxWindowHost(N, K, S, W, A)
    with pytest.raises(api.LdpcAmdError):
        api.FecRxWindowHost(N, N, S, 4, 10)
