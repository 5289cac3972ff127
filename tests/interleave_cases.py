"""Streams and helpers shared by tests/test_interleave_cpu.py, tests/test_interleave_abi.py and tests/test_gpu_interleave.py (numpy and
the package's host side only): the block-interleaved wire of include/ldpc_erasure_amd_interleave.h on n = 200, k = 150, S = 16."""
import os
import sys

import numpy as np

import rxw_cases as rc

sys.path.insert(0, os.path.join(rc.ROOT, "tools"))
import interleave_model as im  # noqa: E402

wm = rc.wm
N, K, S = rc.N, rc.K, rc.S
DEPTHS = im.DEPTHS
# (window, depth) of the lockstep tests: the smallest window of every depth, one that is no multiple of its depth, one far wider
WD = [(2, 1), (4, 2), (8, 4), (9, 4), (16, 8), (32, 16), (32, 4)]
AHEAD = (0, 10)
BLOCK0 = (248, 250)   # a multiple of every depth but 16; off every depth but 1 and 2; both cross the 8-bit wrap


def wire(F, block0, D, n=N):
    """(blk, sym) of the loss-free depth-D wire of F frames numbered from block0."""
    return im.headers(F, n, block0, D)


def frames_for(D):
    """Frames of a lockstep stream: more than two groups, ending inside one."""
    return max(2 * D + D // 2 + 3, 11)


GAP = 72   # blocks of the outage in a lockstep stream: the widest window and its open blocks cannot slide across it by forced closes;
           # with the tail behind it still fewer than the 127 blocks a packet may be ahead


def stream(seed, D, block0, link_window, S=S, F=None):
    """An interleaved stream that mixes what the rule distinguishes: packets thinned at a rate per block, one block of the second
    group nearly lost (a thin group: forced closes), then an outage of GAP whole blocks and one more group and a half (with an
    ahead limit the window empties by forced closes and re-anchors, at a group start below the first block it sees), reordering
    within link_window packet times, duplicates with another payload, foreign block numbers, symbol numbers >= n."""
    rng = np.random.default_rng(seed)
    F = F or frames_for(D)
    b1, s1 = wire(F, block0, D)
    b2, s2 = wire(D + D // 2 + 2, (block0 + F + GAP) & 0xFF, D)
    blk, sym = np.concatenate([b1, b2]), np.concatenate([s1, s2])
    rates = rng.choice([1.0, 0.97, 0.92, 0.85], size=256)
    rates[(block0 + D + 1) & 0xFF] = 0.3
    keep = rng.random(blk.shape[0]) < rates[blk]
    pk = rc.packets_of(blk[keep], sym[keep], S, seed=seed + 2)
    return rc.through_link(pk, seed + 3, link_window, dup=0.03, bad_sym=0.01, foreign=0.02)


def outage_stream(D, F, block0, lo, hi):
    """The loss-free wire with the packets lo .. hi-1 removed: (blk, sym)."""
    blk, sym = wire(F, block0, D)
    keep = np.ones(blk.shape[0], dtype=bool)
    keep[lo:hi] = False
    return blk[keep], sym[keep]


def model(blk, sym, W, A, D, n=N, k=K):
    """The model over the whole stream and its flush: (Window, closed blocks of push_many, closed blocks of flush)."""
    w = wm.Window(n, k, W, A, D)
    closed, used = w.push_many(blk, sym, 1 << 30)
    assert used == len(blk)
    return w, closed, w.flush()


def host_run(pk, W, A, D, max_blocks=1 << 20, cuts=(), n=N, k=K):
    """api.FecRxWindowHost(depth = D) over the stream, fed in the calls the cut positions make, each call repeated until it has
    consumed its piece, then flushed: dict(blocks, sym, er, used (per call), stats, state (before the flush), flushed, stats_end)."""
    from ldpc_erasure_codes_amd import api
    S_ = pk.shape[1] - 8
    blocks, syms, ers, used = [], [np.zeros((0, n, S_), np.uint8)], [np.zeros((0, n), np.uint8)], []
    with api.FecRxWindowHost(n, k, S_, W, A, depth=D) as rx:
        assert rx.depth == D
        edges = [0] + sorted(c for c in cuts if 0 < c < pk.shape[0]) + [pk.shape[0]]
        for a, b in zip(edges[:-1], edges[1:]):
            pos = a
            while pos < b:
                bl, sy, er, u = rx.push_many(pk[pos:b], min(max_blocks, max(1, (b - pos))))
                blocks += bl.tolist()
                syms.append(sy)
                ers.append(er)
                used.append(u)
                pos += u
        out = dict(blocks=blocks, sym=np.concatenate(syms), er=np.concatenate(ers), used=used, stats=rx.stats(), state=rx.state(),
                   dropped=rx.dropped)
        fb, fs, fe = rx.flush()
        out.update(flushed=(fb.tolist(), fs, fe), stats_end=rx.stats(), state_end=rx.state())
        return out


def assert_host_equals_model(h, pk, W, A, D, n=N, k=K):
    blk, sym = wm.headers(pk)
    w = wm.Window(n, k, W, A, D)
    closed, used = w.push_many(blk, sym, 1 << 30)
    mb, ms, me = wm.planes(closed, pk, n)
    assert h["blocks"] == mb.tolist()
    assert np.array_equal(h["sym"], ms) and np.array_equal(h["er"], me)
    assert h["stats"] == w.totals and h["state"] == w.state()
    assert h["dropped"] == w.totals["bad_symbol"] + w.totals["late"] + w.totals["ahead_total"]
    assert sum(h["used"]) == used == pk.shape[0]
    fb, fs, fe = wm.planes(w.flush(), pk, n)
    assert h["flushed"][0] == fb.tolist() and np.array_equal(h["flushed"][1], fs) and np.array_equal(h["flushed"][2], fe)
    assert h["stats_end"] == w.totals and h["state_end"] == w.state()
    return w


def small_cuts(P, seed):
    """Call boundaries a few packets to a few hundred apart."""
    rng = np.random.default_rng(seed)
    cuts, pos = [], 0
    while pos < P:
        pos += int(rng.choice([1, 17, 63, 64, 65, 300, 1111]))
        cuts.append(pos)
    return [c for c in cuts if c < P]


# ---- the plan-edge stream of tests/test_gpu_interleave.py: events placed on chosen lanes of the grouped scan's groups of 64 ----------
EDGE_D, EDGE_W, EDGE_A = 16, 32, 10
EDGE_BLOCK0 = 240


def edge_stream():
    """(blk, sym) at depth 16 from block 240 on: two loss-free groups (240 .. 255, 0 .. 15: every group ends with its 16 blocks
    closing by c == n on 16 adjacent packets, the last of them a g == 1 close, across the 8-bit wrap); then, the window empty, 11
    packets of block 69 = 64 + 5, 53 blocks ahead: a re-anchor at group start 64 with the tripping packet in slot 5, within 27
    packets of the g == 1 close before it; then the loss-free groups 64 .. 79 and 80 .. 95 (block 69 holds n + 1 packets, so it
    closes by the kd clause only when group 80 arrives), a late packet, a bad symbol number, and 17 packets of group 96."""
    D = EDGE_D
    b1, s1 = wire(2 * D, EDGE_BLOCK0, D)
    b2, s2 = wire(2 * D, 64, D)
    b3, s3 = wire(D, 96, D)
    blk = np.concatenate([b1, np.full(11, 69), b2[:5000], [3], [64 + 20], b2[5000:], b3[:17]]).astype(np.int64)
    sym = np.concatenate([s1, np.arange(11), s2[:5000], [7], [0xFFFF], s2[5000:], s3[:17]]).astype(np.int64)
    return blk, sym


def edge_events():
    """[(packet, kind, base)] of the edge stream from the model."""
    blk, sym = edge_stream()
    w = wm.Window(N, K, EDGE_W, EDGE_A, EDGE_D)
    w.push_many(blk, sym, 1 << 30)
    return [(p, kind, b) for (p, kind), b in zip(w.events, w.event_base)]


def edge_calls():
    """Call boundaries [(start, end)] on the edge stream.  With n = 200 and D = 16 a group is 3200 = 50 * 64 packets, so in one call
    from packet 0 the 16 closes of the first group's end sit on lanes 48 .. 63.  The cuts move them: the first group's closes start on
    lane 56 of their call (they straddle a boundary of 64) and its last close is the last packet of a call; a call boundary falls
    inside the second group's 16 closes, whose g == 1 close and the re-anchor behind it lie in one group of 64; a close of the third
    group on lane 0 and a later one on lane 63; a last call of 17 packets."""
    ev = edge_events()
    P = edge_stream()[0].shape[0]
    closes = [p for p, kind, _ in ev if kind == "close"]
    first, second, third = closes[0], closes[16], closes[32]
    cuts = {first - 56 - 64, closes[15] + 1, second + 8, third, closes[40] - 63 - 128, P - 17}
    edges = [0] + sorted(cuts) + [P]
    return list(zip(edges[:-1], edges[1:]))


def edge_facts(calls):
    """What the calls place where, from the model alone: a set of tags."""
    ev = edge_events()
    D = EDGE_D
    facts = set()
    closes = [p for p, kind, _ in ev if kind == "close"]
    runs = [closes[i:i + D] for i in range(len(closes) - D + 1) if closes[i + D - 1] - closes[i] == D - 1]
    for s, e in calls:
        inside = [(p - s, kind, base) for p, kind, base in ev if s <= p < e]
        for q, kind, base in inside:
            if kind == "close" and q % 64 in (0, 63):
                facts.add("close on lane %d" % (q % 64))
            if kind == "close" and s + q + 1 == e:
                facts.add("close on the last packet of a call")
        groups = {}
        for q, kind, base in inside:
            groups.setdefault(q // 64, []).append((kind, base))
        for evs in groups.values():
            if any(kind == "close" and base % D == D - 1 for kind, base in evs) and any(kind == "resync" for kind, _ in evs):
                facts.add("g == 1 close and re-anchor in a group")
        for run in runs:
            if s <= run[0] and run[-1] < e and (run[0] - s) // 64 != (run[-1] - s) // 64:
                facts.add("group-end closes straddle a boundary of 64")
            if run[0] < s <= run[-1]:
                facts.add("group-end closes straddle a call boundary")
        if e - s < 64:
            facts.add("short call")
    blk = edge_stream()[0]
    if any(kind == "resync" and int(blk[p]) % D != 0 for p, kind, _ in ev):
        facts.add("re-anchor into a slot above 0")
    return facts


EDGE_WANT = {"close on lane 0", "close on lane 63", "close on the last packet of a call", "g == 1 close and re-anchor in a group",
             "group-end closes straddle a boundary of 64", "group-end closes straddle a call boundary", "short call",
             "re-anchor into a slot above 0"}
