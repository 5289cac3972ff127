"""The host model of the batch flush (tools/flush_plan.py) against api.FecRx drained flow by flow, and what the stream sets of
tests/test_gpu_flows_flush.py hold, asserted on the reference side alone (no GPU): the four flow kinds a flush can get wrong -- two
open blocks, an empty current block in front of a non-empty next one, nothing open, a block with fewer than k symbols -- must all
be there, so that the GPU tests cannot pass vacuously."""
import os
import sys

import numpy as np
import pytest

from ldpc_erasure_codes_amd import codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flush_plan as fp  # noqa: E402


def _rand():
    from test_gpu_receiver import random_code
    return random_code()


def _drained(rxs, flows, rounds):
    """(slots, closes) of the per-flow loop over host receivers: `rounds` flushes of every listed flow, in list order."""
    slots, closes = [], []
    for f in flows:
        fl = fp.drain(rxs[f], rounds)
        slots += [(f, b) for b, _, _ in fl]
        closes.append(len(fl))
    return slots, np.array(closes, dtype=np.int32)


def test_mixed_stream_set_holds_the_four_flow_kinds(oracle):
    code = _rand()
    for S in (16, 128):                      # (the draws do not depend on S: the same kinds at both)
        sc = fp.scenario("mixed", oracle.OracleCode(code), code, S)
        kd = fp.kinds(sc["flushes"], code.k)
        assert kd["two"] and kd["empty_cur"] and kd["nothing"] and kd["short"], kd
        assert 5 in kd["empty_cur"] and 0 in kd["nothing"] and (6, 0) in kd["short"] and 8 in kd["two"]
        assert [len(fl) for fl in sc["flushes"]][5:] == [2, 1, 1, 2]
        for f, pk in enumerate(sc["flows"]):  # every packet is consumed, call by call
            assert sum(c["flows"][f]["used"] for c in sc["calls"]) == pk.shape[0]


def test_builtin_stream_set_tails(oracle):
    code = codes.load_builtin(1)
    n, k = code.n, code.k
    sc = fp.scenario("builtin", oracle.OracleCode(code), code, 16)
    got = [[(b, int((er == 0).sum())) for b, _, er in fl] for fl in sc["flushes"]]
    assert [len(g) for g in got] == [1, 1, 1, 2]
    assert got[0] == [(1, n - 1)] and got[1][0][0] == 9 and got[2][0][0] == 201
    assert k < got[1][0][1] < n - 408 and k < got[2][0][1] < n - 380       # at least k symbols; more erasures than a block that closes can have
    assert got[3] == [(255, k - 40), (0, 25)]                                # undecodable, across the wrap of the block number


@pytest.mark.parametrize("name", ["mixed", "many", "crowd"])
def test_model_equals_host_receivers_drained_per_flow(oracle, name):
    code = _rand()
    n, k, S = code.n, code.k, 16
    sc = fp.scenario(name, oracle.OracleCode(code), code, S)
    nf = len(sc["flows"])
    assert nf == dict(mixed=9, many=130, crowd=300)[name]
    state = fp.state_of(sc["flushes"])
    per_flow = np.array([len(fl) for fl in sc["flushes"]])
    assert set(per_flow.tolist()) == {0, 1, 2}
    assert [fp.open_blocks(*s) for s in zip(*state)] == per_flow.tolist()
    # a full drain
    pl = fp.plan(state)
    want = [(f, b) for f, fl in enumerate(sc["flushes"]) for b, _, _ in fl]
    assert pl["slots"] == want and np.array_equal(pl["closes"], per_flow) and pl["closes"].dtype == np.int32
    assert all(fp.open_blocks(*s) == 0 for s in zip(*pl["state"]))
    # a subset in its own order, one round; then the rest: the state after the first call decides the second
    rng = np.random.default_rng(5)
    first = [5, 2, 7] if name == "mixed" else rng.permutation(nf)[:nf // 3].tolist()
    rxs = fp.host_receivers(sc, n, k, S)
    p1 = fp.plan(state, first, 1)
    s1, c1 = _drained(rxs, first, 1)
    assert p1["slots"] == s1 and np.array_equal(p1["closes"], c1) and [f for f, _ in s1] == [f for f in first if per_flow[f]]
    untouched = [f for f in range(nf) if f not in first]
    for a, b in zip(p1["state"], state):
        assert np.array_equal(a[untouched], b[untouched])
    p2 = fp.plan(p1["state"], None, 2)
    s2, c2 = _drained(rxs, range(nf), 2)
    assert p2["slots"] == s2 and np.array_equal(p2["closes"], c2)
    assert np.array_equal(c2[first], np.maximum(per_flow[first] - 1, 0)) and np.array_equal(c2[untouched], per_flow[untouched])
    for rx in rxs:
        assert rx.flush() is None
        rx.close()
