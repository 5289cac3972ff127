"""CPU tests of the link emulator's model (tools/link_model.py, the numpy statement of include/ldpc_erasure_amd_link.h): the
windowed-rank form -- the kernel's algorithm, tile and halo included -- against the brute-force sort over the whole plan grid, and
the properties the header promises."""
import numpy as np
import pytest

import link_cases as cases
from link_cases import lm


def case(P, W, seed=None):
    v = cases.cpu_variant(P, W)
    pr = cases.params_of(v, W, seed=1000 * P + W if seed is None else seed)
    return pr, cases.lost_host(v[0], P, v[2])


def test_the_grid_uses_every_variant():
    used = {cases.cpu_variant(P, W) for P, W in cases.GRID}
    assert {v[0] for v in used} == set(cases.LOSTS) and {v[1] for v in used} == set(cases.DUPS)
    assert {v[2] for v in used} == set(cases.FIRSTS) and {v[3] for v in used} == {0.0, 0.005, 0.5}
    assert len(cases.VARIANTS) == 12 and len(cases.GRID) == 56 and (257, 4096) in cases.GRID


@pytest.mark.parametrize("T", [1, 4, 256])
@pytest.mark.parametrize("P,W", cases.GRID)
def test_windowed_rank_is_the_brute_force_sort(P, W, T):
    pr, lost = case(P, W)
    src, fate = lm.plan(pr, P, lost)
    rank, Q = lm.ranks_windowed(pr, P, lost, T)
    d = lm.draws(pr, P, lost)
    assert Q == src.shape[0] == int(d.exists.sum())
    assert np.array_equal(np.sort(rank[rank >= 0]), np.arange(Q))          # a permutation of 0 .. Q-1
    assert np.array_equal(rank >= 0, d.exists)
    w_src, w_fate = lm.plan_windowed(pr, P, lost, T)
    assert np.array_equal(w_src, src) and np.array_equal(w_fate, fate)


@pytest.mark.parametrize("P,W", cases.GRID)
def test_plan_properties(P, W):
    pr, lost = case(P, W)
    d = lm.draws(pr, P, lost)
    src, fate = lm.plan(pr, P, lost)
    survivors = P if lost is None else int((lost == 0).sum())
    copies = int(d.exists[:, 1].sum())
    assert src.shape[0] == survivors + copies                               # Q = survivors + copies
    assert int(((fate & lm.COPY) != 0).sum()) == copies
    if pr.dup == 1.0:
        assert src.shape[0] == 2 * survivors
    if pr.dup == 0.0:
        assert copies == 0
    if lost is not None and lost.all():
        assert src.shape[0] == 0
    assert (d.delay >= 0).all() and (d.delay <= W).all()
    if P and W >= 63 and P > 1:
        assert d.delay.max() > 0
    # no entry of packet i arrives before an entry of a packet <= i - W - 2: the running maximum of what has arrived is never
    # more than W + 1 ahead
    if src.shape[0]:
        ahead = np.maximum.accumulate(src.astype(np.int64)) - src
        assert int(ahead.max()) <= W + 1
    # every arriving packet was sent and survived; the flip flag sits on the copies alone, and only when asked for
    if lost is not None and src.shape[0]:
        assert not lost[src].any()
    flipped = (fate & lm.FLIPPED) != 0
    assert np.array_equal(flipped, ((fate & lm.COPY) != 0) & bool(pr.flags & lm.DUP_FLIP))
    both = (fate & (lm.BADSYM | lm.FOREIGN)) == (lm.BADSYM | lm.FOREIGN)
    assert not both.any() and not (fate[(fate & lm.FOREIGN) == 0] >> 8).any()
    if pr.bad_sym == 0.5 and src.shape[0] > 100:
        assert ((fate & lm.BADSYM) != 0).any() and ((fate & lm.FOREIGN) != 0).any()
        assert (((fate & lm.BADSYM) != 0) | ((fate & lm.FOREIGN) != 0)).all()   # 0.5 + 0.5: every entry is damaged


def test_a_pristine_link_changes_nothing():
    P, S = 300, 16
    pr = lm.Params(seed=5)
    src, fate = lm.plan(pr, P)
    assert np.array_equal(src, np.arange(P)) and not fate.any()
    pk = cases.random_packets(np.random.default_rng(1), P, S)
    out, fo = lm.apply(pk, src, fate, flow_of=np.arange(P, dtype=np.int32) % 3)
    assert np.array_equal(out, pk) and np.array_equal(fo, np.arange(P) % 3)
    off = np.arange(P + 1, dtype=np.int64) * (8 + S)
    by, o = lm.apply_ragged(pk.reshape(-1), off, src, fate)
    assert np.array_equal(by, pk.reshape(-1)) and np.array_equal(o, off)


@pytest.mark.parametrize("first", cases.FIRSTS)
def test_two_calls_make_the_draws_of_one(first):
    """Two calls of P1 and P2 packets with first advanced make the same DRAWS as one call of P1 + P2 packets -- the same fates and
    delays per entry.  Packets do not cross a call boundary: the arrival orders differ near the seam."""
    P1, P2, W = 300, 212, 40
    pr = lm.Params(seed=9, first=first, window=W, flags=lm.DUP_FLIP, dup=0.3, bad_sym=0.1, foreign=0.2)
    lost = cases.lost_host("uniform", P1 + P2, first)
    one = lm.draws(pr, P1 + P2, lost)
    a = lm.draws(pr, P1, lost[:P1])
    b = lm.draws(pr._replace(first=first + P1), P2, lost[P1:])
    for name in ("exists", "delay", "fate"):
        assert np.array_equal(np.concatenate([getattr(a, name), getattr(b, name)]), getattr(one, name)), name
    assert np.array_equal(np.concatenate([a.time, b.time + P1]), one.time)
    src_a, _ = lm.plan(pr, P1, lost[:P1])
    src_b, _ = lm.plan(pr._replace(first=first + P1), P2, lost[P1:])
    src_one, _ = lm.plan(pr, P1 + P2, lost)
    two = np.concatenate([src_a, src_b + P1])
    assert np.array_equal(np.sort(two), np.sort(src_one))                   # the same packets arrive ...
    assert (src_a < P1).all() and not np.array_equal(two, src_one)          # ... none across the boundary, where one call re-orders


def test_foreign_block_values_are_not_constant():
    """The regression test of the block value's draw: taken from the top byte of the damage draw it would be small whenever the
    entry is FOREIGN at a small probability (the top byte IS the compare's leading byte)."""
    P = 20000
    pr = lm.Params(seed=3, foreign=0.01)
    _, fate = lm.plan(pr, P)
    blocks = (fate[(fate & lm.FOREIGN) != 0] >> 8).astype(int)
    assert blocks.shape[0] > 100
    assert len(set(blocks.tolist())) > 50 and blocks.max() > 200 and blocks.min() < 50
    # with bad_sym in front the FOREIGN band of r is [t_bad, t_bad + t_foreign): still every value
    _, fate = lm.plan(pr._replace(bad_sym=0.3), P)
    blocks = (fate[(fate & lm.FOREIGN) != 0] >> 8).astype(int)
    assert len(set(blocks.tolist())) > 50


def test_damage_touches_the_stated_bytes_only():
    pk = np.arange(8 + 12, dtype=np.uint8) + 1
    assert np.array_equal(lm.damage(pk, 0), pk) and np.array_equal(lm.damage(pk, lm.COPY), pk)
    bad = lm.damage(pk, lm.BADSYM)
    assert (bad[[0, 1, 4, 5]] == 0xFF).all() and np.array_equal(np.delete(bad, [0, 1, 4, 5]), np.delete(pk, [0, 1, 4, 5]))
    fo = lm.damage(pk, lm.FOREIGN | 0xAB << 8)
    assert (fo[[2, 6]] == 0xAB).all() and np.array_equal(np.delete(fo, [2, 6]), np.delete(pk, [2, 6]))
    fl = lm.damage(pk, lm.COPY | lm.FLIPPED)
    assert np.array_equal(fl[:8], pk[:8]) and np.array_equal(fl[8:], pk[8:] ^ 0x5A)
    assert np.array_equal(lm.badsym_slot(20), lm.damage(np.zeros(20, dtype=np.uint8), lm.BADSYM))


def test_apply_ragged_vets_the_boundaries_and_sums_the_lengths():
    rng = np.random.default_rng(4)
    ln = np.array([8, 30, 7, 12, 9, 100, 8], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    off[4] = off[3] - 2                      # datagram 3 runs backwards (and datagram 4 grows by what it lost)
    data = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    src = np.array([6, 5, 2, 3, 0, 0, -1, 7, 1, 4], dtype=np.int32)
    fate = np.array([0, lm.BADSYM, 0, 0, lm.COPY | lm.FLIPPED, lm.FOREIGN | 0x77 << 8, 0, 0, 0, 0], dtype=np.uint16)
    by, o = lm.apply_ragged(data, off, src, fate)
    want_len = [8, 100, 0, 0, 8, 8, 0, 0, 30, int(off[5] - off[4])]
    assert np.array_equal(np.diff(o), want_len) and o[0] == 0 and o[-1] == by.shape[0]
    assert np.array_equal(by[o[0]:o[1]], data[off[6]:off[7]])
    assert np.array_equal(by[o[1]:o[2]], lm.damage(data[off[5]:off[6]], lm.BADSYM))
    assert np.array_equal(by[o[4]:o[5]], data[0:8]) and np.array_equal(by[o[5]:o[6]], lm.damage(data[0:8], lm.FOREIGN | 0x77 << 8))
    # a datagram that would end beyond bytes_cap is not written, the sums still count it
    by2, o2 = lm.apply_ragged(data, off, src, fate, bytes_cap=int(o[2]) - 1)
    assert np.array_equal(o2, o) and not by2[o[1]:o[2]].any() and np.array_equal(by2[:o[1]], by[:o[1]])


def _closes_and_decodes(oracle, code, S, F, packets, arrived, block0):
    """The host reference alone: every block but the last open one is closed by the stream itself, in order, and the oracle decodes
    all of them (message passing and the ML stage, on the patterns)."""
    from oracle import oracle_py
    blocks, _, er, dropped, flushed = cases.host_receiver(arrived, code.n, code.k, S, F + 2)
    assert blocks.tolist() == [(block0 + f) & 0xFF for f in range(F)] and flushed == 1
    assert (er.sum(axis=1) > 0).all() and dropped > 0
    _, _, _, st = oracle_py.OracleCode(code).decode_batch_s1(np.zeros((F, code.n), dtype=np.uint8), er)
    assert (st <= 1).all(), st


def test_the_end_to_end_inputs_close_and_decode_on_the_host_reference(oracle, code_a):
    from code_helpers import random_code
    from ldpc_erasure_codes_amd import api
    e = cases.E2E_FIXED
    assert (code_a.n, code_a.k) == (2040, 1530)
    pk = api.fec_packetize(np.zeros((e["F"], code_a.n, e["S"]), dtype=np.uint8), 1, 0)
    out, _, src, fate, lost = cases.e2e_model(pk, cases.e2e_params(e["seed"]), e["loss_seed"], e["loss"])
    assert 0.03 < lost.mean() < 0.07 and ((fate & lm.BADSYM) != 0).any() and ((fate & lm.FOREIGN) != 0).any() and ((fate & lm.FLIPPED) != 0).any()
    assert (np.diff(src) < 0).any()
    _closes_and_decodes(oracle, code_a, e["S"], e["F"], pk, out, 0)
    e = cases.E2E_FLOWS
    code = random_code()
    nf, per = e["nflows"], e["per"]
    pks = [api.fec_packetize(np.zeros((per, code.n, e["S"]), dtype=np.uint8), 1, b0) for b0 in e["block0"]]
    pk = np.stack(pks, axis=1).reshape(nf * per * code.n, 8 + e["S"])                  # one packet of every flow in turn
    flow_of = np.tile(np.arange(nf, dtype=np.int32), per * code.n)
    out, fo, _, _, _ = cases.e2e_model(pk, cases.e2e_params(e["seed"], window=e["window"]), e["loss_seed"], e["loss"], flow_of)
    for f in range(nf):
        _closes_and_decodes(oracle, code, e["S"], per, pks[f], out[fo == f], e["block0"][f])
