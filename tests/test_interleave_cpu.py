"""The block-interleaved wire without a GPU (include/ldpc_erasure_amd_interleave.h): the layout (C against numpy), the depth-D rule of
the windowed receiver -- the C host object (csrc/rx_window.cpp) against the numpy model (tools/rx_window_model.py) --, the facts the
rule is built on, and what interleaving buys on the bursty channel (model + CPU oracle).  Streams: tests/interleave_cases.py."""
import ctypes as C

import numpy as np
import pytest

import interleave_cases as ic
import rxw_cases as rc
from code_helpers import random_code
from ldpc_erasure_codes_amd import api, synth

wm, im = ic.wm, ic.im
N, K, S = ic.N, ic.K, ic.S
EINVAL = -1


# ------------------------------------------------------------------------------------------------------ 1. the layout
@pytest.mark.parametrize("D", ic.DEPTHS)
@pytest.mark.parametrize("F,block0", [(11, 250), (600, 250), (600, 0), (1, 255), (0, 3)])
def test_layout_equals_the_numpy_statement_and_is_a_permutation(F, block0, D):
    first, stride = api.fec_tx_ilv_layout(F, N, block0, D)
    mf, ms = im.layout(F, N, block0, D)
    assert first.dtype == np.int64 and stride.dtype == np.int32
    assert np.array_equal(first, mf) and np.array_equal(stride, ms)
    pos = (first[:, None] + np.arange(N)[None, :] * stride[:, None]).ravel()
    assert np.array_equal(np.sort(pos), np.arange(F * N)), "every wire position is taken once"
    if D == 1:
        assert np.array_equal(first, np.arange(F) * N) and (stride == 1).all(), "depth 1 is the straight sender's order"
    # the statement itself: frames of one group, consecutive, share a run; row j of member i of the run s .. s+m-1 is n s + j m + i
    blocks = (block0 + np.arange(F)) & 0xFF
    s = 0
    while s < F:
        m = min(D - blocks[s] % D, F - s)
        assert np.array_equal(first[s:s + m], s * N + np.arange(m)) and (stride[s:s + m] == m).all()
        assert np.unique(blocks[s:s + m] // D).size == 1
        s += m


def test_layout_partial_runs_and_the_wrap():
    """F = 11 from block 250 at depth 4: blocks 250 251 | 252 .. 255 | 0 .. 3 | 4 -- a short first run, the wrap between two full
    runs, a short last run."""
    first, stride = api.fec_tx_ilv_layout(11, N, 250, 4)
    assert stride.tolist() == [2, 2, 4, 4, 4, 4, 4, 4, 4, 4, 1]
    assert first.tolist() == [0, 1, 2 * N, 2 * N + 1, 2 * N + 2, 2 * N + 3, 6 * N, 6 * N + 1, 6 * N + 2, 6 * N + 3, 10 * N]
    blk, sym = im.headers(11, N, 250, 4)
    assert blk[:4].tolist() == [250, 251, 250, 251] and sym[:4].tolist() == [0, 0, 1, 1]
    assert blk[2 * N:2 * N + 5].tolist() == [252, 253, 254, 255, 252]


def test_layout_refusals():
    L = api.load_library()
    f = L.ldpc_amd_fec_tx_ilv_layout
    assert f(4, N, 0, 4, None, None) == 4 * N, "first and stride may be NULL"
    for depth in (0, 3, 5, 6, 12, 32, -1):
        assert f(4, N, 0, depth, None, None) == EINVAL
    assert f(4, 0, 0, 4, None, None) == EINVAL and f(4, -1, 0, 4, None, None) == EINVAL
    assert f(-1, N, 0, 4, None, None) == EINVAL
    assert f((1 << 31) // N + 1, N, 0, 4, None, None) == EINVAL, "nframes * n >= 2^31"
    most = ((1 << 31) - 1) // N
    assert f(most, N, 0, 16, None, None) == most * N and f(1 << 31, 1, 0, 1, None, None) == EINVAL
    with pytest.raises(api.LdpcAmdError):
        api.fec_tx_ilv_layout(4, N, 0, 3)


# ------------------------------------------------------------------------------------------------------ 2. host object == model
@pytest.mark.parametrize("block0", ic.BLOCK0)
@pytest.mark.parametrize("W,D", ic.WD)
def test_host_equals_model_on_interleaved_streams(W, D, block0):
    seen = dict(resyncs=0, forced=0, bad=0, dup=0, late=0)
    for A in ic.AHEAD:
        for i, lw in enumerate((0, 150, 400)):
            pk = ic.stream(1000 + 7 * D + i, D, block0, lw)
            cuts = ic.small_cuts(pk.shape[0], 3 + i)
            h = ic.host_run(pk, W, A, D, max_blocks=(1, 2, 3)[i], cuts=cuts)
            w = ic.assert_host_equals_model(h, pk, W, A, D)
            blk, sym = wm.headers(pk)
            seen["resyncs"] += w.totals["resyncs"]
            seen["forced"] += w.totals["ahead_total"] > A > 0
            seen["bad"] += w.totals["bad_symbol"]
            seen["late"] += w.totals["late"]
            seen["dup"] += pk.shape[0] - np.unique(np.stack([blk, sym]), axis=1).shape[1]
            # (without an ahead limit the thin block, or a leading empty slot, stalls the window)
            assert len(h["blocks"]) + len(h["flushed"][0]) >= ic.frames_for(D) - 1 or A == 0
    assert seen["forced"] >= 1 and seen["bad"] > 0 and seen["dup"] > 0 and seen["late"] > 0, seen
    assert seen["resyncs"] >= 3, "every stream re-anchors behind its outage when there is an ahead limit"


@pytest.mark.parametrize("W,D", [(8, 4), (32, 16)])
def test_host_equals_model_packet_by_packet(W, D):
    pk = ic.stream(77, D, 250, 150)
    blk, sym = wm.headers(pk)
    w = wm.Window(N, K, W, 10, D)
    with api.FecRxWindowHost(N, K, S, W, 10, depth=D) as rx:
        for p in range(pk.shape[0]):
            r, h = w.push(int(blk[p]), int(sym[p])), rx.push(pk[p])
            assert (r is None) == (h is None), p
            if r is not None:
                _, ms, me = wm.planes([r], pk, N)
                assert h[0] == r[0] and np.array_equal(h[1], ms[0]) and np.array_equal(h[2], me[0]), p
            if p % 97 == 0 or r is not None:
                assert rx.state() == w.state() and rx.stats() == w.totals, p


# ------------------------------------------------------------------------------------------------------ 3. the facts
@pytest.mark.parametrize("D,W", [(2, 4), (4, 8), (8, 16), (16, 32)])
def test_a_loss_free_interleaved_stream_keeps_every_row(D, W):
    """(a) 40 blocks from block 240 (a group start at every depth, the 8-bit wrap inside): the depth-D object hands out n rows per
    block and drops nothing; the plain object on the same wire closes its blocks just past km and drops the rest of their rows as
    late."""
    blk, sym = ic.wire(40, 240, D)
    pk = rc.packets_of(blk, sym)
    h = ic.host_run(pk, W, 10, D)
    ic.assert_host_equals_model(h, pk, W, 10, D)
    er = np.concatenate([h["er"], h["flushed"][2]])
    blocks = h["blocks"] + h["flushed"][0]
    got = [(b, int(N - e.sum())) for b, e in zip(blocks, er) if not e.all()]
    assert got == [((240 + f) & 0xFF, N) for f in range(40)]
    assert h["stats_end"]["late"] == 0 and h["stats_end"]["ahead_total"] == 0 and h["stats_end"]["resyncs"] == 0
    old = ic.host_run(pk, W, 10, 1)
    rows = N - np.concatenate([old["er"], old["flushed"][2]]).sum(axis=1)
    assert old["stats_end"]["late"] > 500 and rows[rows > 0].min() == rc.KM + 1, "the plain rule on the interleaved wire"


@pytest.mark.parametrize("lost", [1, 2, 3, 5])
def test_lost_leading_packets_cost_no_block(lost):
    """(b) An aligned stream (block 248, depth 8) whose first packets are lost: base is the group start and every block comes out."""
    D, W = 8, 16
    blk, sym = ic.wire(24, 248, D)
    pk = rc.packets_of(blk[lost:], sym[lost:])
    with api.FecRxWindowHost(N, K, S, W, 10, depth=D) as rx:
        assert rx.push(pk[0]) is None
        assert int(blk[lost]) != 248 and rx.state()["base"] == 248
    h = ic.host_run(pk, W, 10, D)
    ic.assert_host_equals_model(h, pk, W, 10, D)
    blocks = h["blocks"] + h["flushed"][0]
    rows = N - np.concatenate([h["er"], h["flushed"][2]]).sum(axis=1)
    assert blocks == [(248 + f) & 0xFF for f in range(24)] and rows.min() >= N - 1 and h["stats_end"]["late"] == 0


def test_a_start_off_the_group_hands_out_leading_erased_blocks():
    """(c) Depth 8 from block 250: the window anchors at 248; blocks 248 and 249 never receive a packet and come out all erased,
    through the ahead limit."""
    D, W, A = 8, 16, 10
    blk, sym = ic.wire(30, 250, D)
    pk = rc.packets_of(blk, sym)
    h = ic.host_run(pk, W, A, D)
    w = ic.assert_host_equals_model(h, pk, W, A, D)
    assert h["blocks"][:3] == [248, 249, 250] and h["er"][0].all() and h["er"][1].all() and not h["er"][2].any()
    forced = [p for (p, kind), b in zip(w.events, w.event_base) if b in (248, 249)]
    # each of the two forced closes takes A + 1 ahead packets; the closes of the full blocks behind them follow packet by packet, and
    # the packets of the third group that pass meanwhile are ahead too: at most one per block of the first group
    assert len(forced) == 2 and 2 * (A + 1) <= h["stats_end"]["ahead_total"] <= 2 * (A + 1) + D
    rows = N - np.concatenate([h["er"], h["flushed"][2]]).sum(axis=1)
    assert sorted(rows.tolist())[:2] == [0, 0] and rows.sum() == pk.shape[0] - h["stats_end"]["ahead_total"] and h["stats_end"]["late"] == 0
    with api.FecRxWindowHost(N, K, S, W, 0, depth=D) as rx:   # A = 0: no forced close, only a flush hands them out
        bl, sy, er, used = rx.push_many(pk, 64)
        assert len(bl) == 0 and used == pk.shape[0]
        fb, _, fe = rx.flush()
        assert fb.tolist()[:2] == [248, 249] and fe[0].all() and fe[1].all()


def test_an_outage_re_anchors_at_the_group_start():
    """(d) Depth 8, 64 blocks from 0, an outage from inside group 2 to inside group 5: one re-anchor, base = the start of the tripping
    packet's group, the packet itself in slot blk mod D."""
    D, W, A = 8, 16, 10
    lo, hi = N * D * 2 + 500, N * D * 5 + 900
    blk, sym = ic.outage_stream(D, 64, 0, lo, hi)
    pk = rc.packets_of(blk, sym)
    h = ic.host_run(pk, W, A, D)
    w = ic.assert_host_equals_model(h, pk, W, A, D)
    assert w.totals["resyncs"] == 1
    (p, kind), = [e for e in w.events if e[1] == "resync"]
    trip = int(blk[p])
    assert trip // D == 5 and trip % D != 0
    w2 = wm.Window(N, K, W, A, D)
    w2.push_many(blk[:p + 1], sym[:p + 1], 1 << 30)
    cnt = [0] * W
    cnt[trip % D] = 1
    assert w2.state() == dict(base=40, cnt=cnt, ahead=0)
    with api.FecRxWindowHost(N, K, S, W, A, depth=D) as rx:
        rx.push_many(pk[:p + 1], 64)
        assert rx.state() == w2.state()
    blocks = h["blocks"] + h["flushed"][0]
    rows = N - np.concatenate([h["er"], h["flushed"][2]]).sum(axis=1)
    # the two thin groups (2 and 5, cut by the outage) leave by forced closes: D (A + 1) ahead packets each, and A + 1 for the re-anchor
    assert w.totals["ahead_total"] == (2 * D + 1) * (A + 1) and w.totals["late"] == 0
    assert [b for b in blocks if b >= 48] == list(range(48, 64)) and all(r == N for b, r in zip(blocks, rows) if 48 <= b < 56 or b < 16)
    assert sum(r for b, r in zip(blocks, rows) if b >= 56) == D * N - D * (A + 1), "group 7 paid for the thin group 5"


def rxw_streams():
    for seed in rc.RANDOM_SEEDS:
        yield rc.random_stream(seed)
    yield rc.random_stream(**rc.WRAP)
    for A in rc.EDGE_A:
        yield rc.packets_of(*rc.edge_stream(A))


def test_depth_1_is_the_plain_object():
    """(e) create_depth(..., 1) == create on every stream of tests/rxw_cases.py."""
    for i, pk in enumerate(rxw_streams()):
        for W, A in rc.WA[i % 2::2]:
            old = rc.host_run(pk, W, A, max_blocks=3)
            new = ic.host_run(pk, W, A, 1, max_blocks=3)
            for key in ("blocks", "used", "stats", "state", "dropped"):
                assert old[key] == new[key], (i, W, A, key)
            assert np.array_equal(old["sym"], new["sym"]) and np.array_equal(old["er"], new["er"])
            m = wm.run(*wm.headers(pk), N, K, W, A)
            md = wm.run(*wm.headers(pk), N, K, W, A, D=1)
            assert m == md


def test_create_refusals():
    """(f)"""
    L = api.load_library()
    h = C.c_void_p()
    for depth in (0, 3, 5, 12, 32, -2):
        assert L.ldpc_amd_fec_rxw_create_depth(N, K, S, 32, 10, depth, C.byref(h)) == EINVAL
    for W, D in [(3, 2), (7, 4), (15, 8), (31, 16), (16, 16), (2, 2)]:
        assert L.ldpc_amd_fec_rxw_create_depth(N, K, S, W, 10, D, C.byref(h)) == EINVAL, "2 * depth > window"
        with pytest.raises(api.LdpcAmdError):
            api.FecRxWindowHost(N, K, S, W, 10, depth=D)
    for W, A in [(1, 0), (33, 0), (4, -1)]:
        assert L.ldpc_amd_fec_rxw_create_depth(N, K, S, W, A, 1, C.byref(h)) == EINVAL
    assert L.ldpc_amd_fec_rxw_depth(None) == -1
    for W, D in [(2, 1), (4, 2), (32, 16), (9, 4)]:
        with api.FecRxWindowHost(N, K, S, W, 10, depth=D) as rx:
            assert rx.depth == D
    with api.FecRxWindowHost(N, K, S, 4, 10) as rx:
        assert rx.depth == 1


def test_plan_edge_stream_places_its_events():
    """The stream and the call boundaries of the GPU plan-edge test do what that test is for -- on the model alone -- and the host
    object agrees with the model on them."""
    calls = ic.edge_calls()
    facts = ic.edge_facts(calls)
    assert ic.EDGE_WANT <= facts, ic.EDGE_WANT - facts
    blk, sym = ic.edge_stream()
    pk = rc.packets_of(blk, sym)
    h = ic.host_run(pk, ic.EDGE_W, ic.EDGE_A, ic.EDGE_D, cuts=[s for s, _ in calls])
    w = ic.assert_host_equals_model(h, pk, ic.EDGE_W, ic.EDGE_A, ic.EDGE_D)
    assert h["blocks"] == [(240 + f) & 0xFF for f in range(32)] + list(range(64, 96)) and w.totals["resyncs"] == 1
    assert w.totals["bad_symbol"] == 1 and w.totals["late"] == 1 and w.totals["ahead_total"] == ic.EDGE_A + 1


# ------------------------------------------------------------------------------------------------------ 4. the burst table
BURST_W, BURST_A, BURST_F, BURST_BLOCK0 = 16, 10, 32, 248


def burst_lost(seed, P):
    """The loss flags by wire position: the Gilbert-Elliott channel of cfg 3, mean bad-state run 10."""
    return synth.erasures_bursty(seed, 0, P, 1, 0.13, 0.8, 10.0).reshape(-1).astype(bool)


def burst_trial(oc, n, k, seed, D):
    """(blocks decoded, rows of the thinnest block handed out with any row, ahead drops) of the model + the oracle."""
    blk, sym = im.headers(BURST_F, n, BURST_BLOCK0, D)
    lost = burst_lost(seed, blk.shape[0])
    w, closed, flushed = ic.model(blk[~lost], sym[~lost], BURST_W, BURST_A, D, n, k)
    closed = closed + flushed
    er = np.ones((len(closed), n), np.uint8)
    for j, (_, win) in enumerate(closed):
        er[j, list(win.keys())] = 0
    _, _, _, st = oc.decode_batch_s1(np.zeros(er.shape, np.uint8), er, itenum=10, do_ml=1)
    sent = {(BURST_BLOCK0 + f) & 0xFF for f in range(BURST_F)}
    good = sum(int(s <= 1) for (b, _), s in zip(closed, np.asarray(st)) if b in sent)
    return good, min(len(win) for _, win in closed if win), w.totals["ahead_total"]


@pytest.mark.parametrize("seed,want", [(79, {1: (30, 193, 22), 4: (32, 217), 8: (32, 224)}), (82, {1: (30, 195, 33), 4: (32, 227), 8: (32, 219)})])
def test_burst_table(oracle, seed, want):
    """code_helpers.random_code() (300,200), 32 frames from block 248, W = 16, A = 10, no reordering: at depth 1 two blocks are lost
    to the bursts, at depth 4 and 8 all 32 decode.  The counts are those of DESIGN.md."""
    code = random_code()
    oc = oracle.OracleCode(code)
    for D, w in want.items():
        got = burst_trial(oc, code.n, code.k, seed, D)
        assert got[:len(w)] == w, (seed, D, got)
    assert want[1][0] < BURST_F == want[8][0]
