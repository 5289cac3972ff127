"""The close rule of the windowed receiver as a value (include/ldpc_erasure_amd_rx_rule.h), without a GPU: the C host object
(api.FecRxWindowHost(rule=)) against the numpy model (tools/rx_window_model.py, rule=) under every rule of tests/rx_rule_cases.py;
the default rule spelled out against the object made without a rule; the MDS rule's plan-edge stream; and the claim the rule exists
for -- on Reed-Solomon shaped blocks behind the burst channel every decodable block is handed out decodable, which the default rule
does not do."""
import numpy as np
import pytest

import rx_rule_cases as rr
from ldpc_erasure_codes_amd import api

rc, wm = rr.rc, rr.wm
N, K, S = rr.N, rr.K, rr.S
WA = [(2, 10), (3, 10), (8, 3), (16, 10)]   # a subset of rc.WA
DEPTH4 = [(8, 10), (16, 10)]                # (W, A) at D = 4

_STREAMS = {}


def stream(seed):
    if seed not in _STREAMS:
        _STREAMS[seed] = rc.random_stream(**rr.WRAP) if seed == "wrap" else rc.random_stream(seed)
    return _STREAMS[seed]


def same_as_model(h, m, pk, tag):
    """Block numbers, winning symbols (as bytes and flags), totals and state of a host run against a model Result."""
    mb, msym, mer = wm.planes(m.closed, pk, N)
    assert h["blocks"] == mb.tolist(), tag
    assert np.array_equal(h["sym"], msym) and np.array_equal(h["er"], mer), tag
    assert h["stats"] == m.totals and h["state"] == m.state, tag
    assert sum(h["used"]) == pk.shape[0] == m.consumed, tag


@pytest.mark.parametrize("name", rr.RULE_NAMES)
@pytest.mark.parametrize("D,WAs", [(1, WA), (4, DEPTH4)])
def test_host_equals_model(name, D, WAs):
    rule = rr.rules(D)[name]
    for seed in rr.RANDOM_SEEDS + ["wrap"]:
        pk = stream(seed)
        rng = np.random.default_rng(17)
        cuts = sorted(int(c) for c in rng.integers(1, pk.shape[0], size=6))
        for W, A in WAs:
            m = rr.model_run(pk, W, A, D, rule)
            tag = (name, D, seed, W, A)
            h = rr.host_run(pk, W, A, D, rule)
            assert h["rule"] == tuple(rule), tag
            same_as_model(h, m, pk, tag)
            same_as_model(rr.host_run(pk, W, A, D, rule, cuts=cuts, max_blocks=2), m, pk, tag + ("split",))


def test_rules_differ_on_the_streams():
    """The comparison above is not one stream of results five times: the rules close different blocks at different packets."""
    pk = stream(rr.RANDOM_SEEDS[0])
    blk, sym = wm.headers(pk)
    ev = {name: tuple(wm.events(blk, sym, N, K, 16, 10, rule=rule)) for name, rule in rr.rules().items()}
    assert len(set(ev.values())) == len(ev)
    late = {name: rr.model_run(pk, 16, 10, 1, rule).totals["late"] for name, rule in rr.rules().items()}
    assert late["at_k"] > late["default"], "closing at the k-th symbol turns the block's remaining packets into late ones"


@pytest.mark.parametrize("D,W,A", [(1, 2, 0), (1, 4, 10), (1, 32, 1), (4, 8, 10)])
def test_spelled_out_default_rule_is_the_object_without_a_rule(D, W, A):
    rule = api.fec_rx_rule_default(N, K)
    assert rule == wm.default_rule(N, K) == (rc.KD + 1, 11, rc.KM + 1, 101)
    for seed in rr.RANDOM_SEEDS[:4] + ["wrap"]:
        pk = stream(seed)
        a, b = rr.host_run(pk, W, A, D, None, flush=True), rr.host_run(pk, W, A, D, rule, flush=True)
        assert a["rule"] == b["rule"] == rule
        for key in ("blocks", "used", "stats", "state", "dropped"):
            assert a[key] == b[key], (seed, key)
        assert np.array_equal(a["sym"], b["sym"]) and np.array_equal(a["er"], b["er"]), seed
    if D == 1:   # and both are the object the plain create call makes, tests/rxw_cases.py's
        c = rc.host_run(stream(rr.RANDOM_SEEDS[0]), W, A)
        d = rr.host_run(stream(rr.RANDOM_SEEDS[0]), W, A, 1, rule)
        assert c["blocks"] == d["blocks"] and np.array_equal(c["sym"], d["sym"]) and c["stats"] == d["stats"] and c["state"] == d["state"]


@pytest.mark.parametrize("A", rr.EDGE_A)
@pytest.mark.parametrize("D,W", rr.EDGE_DEPTH)
def test_mds_edge_stream_places_its_events(D, W, A):
    """What tests/test_gpu_rx_rule.py relies on, from the model alone; and the host object follows the model over those calls."""
    blk, sym = rr.edge_stream(A)
    calls = rr.edge_calls(blk, sym, W, A, D)
    facts = rr.edge_facts(blk, sym, W, A, D, calls)
    assert rr.edge_facts_wanted(W, A, D) <= facts, (rr.edge_facts_wanted(W, A, D) - facts)
    pk = rc.packets_of(blk, sym)
    rule = wm.mds_rule(N, K, D)
    m = rr.model_run(pk, W, A, D, rule)
    assert any(len(win) == 0 for _, win in m.closed) or D > 1, "an all-erased block is handed out"
    same_as_model(rr.host_run(pk, W, A, D, rule, cuts=[s for s, _ in calls], max_blocks=64), m, pk, (D, W, A))


def test_all_facts_on_the_wide_window():
    """W = 16, A = 10 shows every item at depth 1; D = 4, W = 8 the cascade behind a give-up close in the grouped form."""
    every = {"give-up close of an empty slot 0", "give-up close and three closes behind it in one group", "lane0", "lane63",
             "last packet of a call", "re-anchor under c_lo == 0", "block numbers wrap", "short call"}
    assert every <= rr.edge_facts_wanted(16, 10, 1)
    assert "give-up close and three closes behind it in one group" in rr.edge_facts_wanted(8, 10, 4)


# ---- the quality claim -----------------------------------------------------------------------------------------------------------------
def host_delivered(blk, sym, W, A, D, rule):
    """(blocks handed out with k or more symbols, totals) of the host object over the stream and its flush."""
    n, k = rr.RS_N, rr.RS_K
    pk = rc.packets_of(blk, sym, S=4)
    with api.FecRxWindowHost(n, k, 4, W, A, depth=D, rule=rule) as rx:
        _, _, er, used = rx.push_many(pk, 1 << 20)
        assert used == pk.shape[0]
        _, _, fer = rx.flush()
        return int(((n - np.concatenate([er, fer]).sum(axis=1, dtype=np.int64)) >= k).sum()), rx.stats()


@pytest.mark.parametrize("seed", rr.QUALITY_SEEDS)
@pytest.mark.parametrize("D,W", rr.QUALITY_DW)
def test_mds_rule_hands_out_every_decodable_block(seed, D, W):
    """RS(255,192)-shaped blocks, 256 of them, in order at depth D behind the Gilbert-Elliott trace of the README's RS row, A = 10,
    flush at the end.  Under the MDS rule every block of which k or more packets arrived is handed out with k or more symbols and no
    packet is dropped ahead of the window; under the default rule strictly fewer are -- by the model and by the host object."""
    n, k, A = rr.RS_N, rr.RS_K, rr.QUALITY_A
    blk, sym, arrived = rr.quality_stream(seed, D)
    decodable = int((arrived >= k).sum())
    assert 0 < decodable < rr.QUALITY_BLOCKS
    got = {}
    for name, rule in (("default", None), ("mds", wm.mds_rule(n, k, D))):
        w = wm.Window(n, k, W, A, D, rule)
        closed, used = w.push_many(blk, sym, 1 << 30)
        closed += w.flush()
        host, totals = host_delivered(blk, sym, W, A, D, rule)
        print(f"seed {seed} D {D} W {W} {name}: model {rr.delivered(closed)} host {host} decodable {decodable} totals {w.totals}")
        assert host == rr.delivered(closed) and totals == w.totals, name
        got[name] = (host, totals)
    assert got["mds"][0] == decodable
    assert got["mds"][1]["ahead_total"] == 0 and got["mds"][1]["late"] == 0
    assert got["default"][0] < decodable, "the default rule's forced closes cost decodable blocks"
