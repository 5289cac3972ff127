"""Streams and helpers shared by tests/test_rx_window_cpu.py, tests/test_rx_window_abi.py and tests/test_gpu_rx_window.py (numpy
and the package's host side only): the windowed receiver of include/ldpc_erasure_amd_rx_window.h on n = 200, k = 150, S = 16."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import link_model as lm  # noqa: E402
import rx_window_model as wm  # noqa: E402

N, K, S = 200, 150, 16
KD, KM = wm.thresholds(N, K)   # 190, 160


def packets_of(blk, sym, S=S, seed=0):
    """Packets uint8 [P][8 + S] with the given headers (both halves, class 1) and a random payload."""
    blk, sym = np.asarray(blk, dtype=np.int64), np.asarray(sym, dtype=np.int64)
    P = blk.shape[0]
    pk = np.random.default_rng(seed).integers(0, 256, size=(P, 8 + S), dtype=np.uint8)
    pk[:, 0], pk[:, 1], pk[:, 2], pk[:, 3] = sym & 0xFF, (sym >> 8) & 0xFF, blk & 0xFF, 1
    pk[:, 4:8] = pk[:, 0:4]
    return pk


def sent(nblocks, keep, seed, block0=0, n=N):
    """The in-order stream of nblocks blocks numbered from block0 (mod 256); keep(b) = the fraction of block b's packets kept.
    Returns (blk, sym)."""
    rng = np.random.default_rng(seed)
    blk, sym = [], []
    for b in range(nblocks):
        m = np.flatnonzero(rng.random(n) < keep(b))
        blk.append(np.full(m.shape[0], (block0 + b) & 0xFF, dtype=np.int64))
        sym.append(m.astype(np.int64))
    return np.concatenate(blk), np.concatenate(sym)


def through_link(pk, seed, window, dup=0.0, bad_sym=0.0, foreign=0.0, dup_flip=True):
    """Packets through tools/link_model.py's link: reordered within `window` packet times, duplicated (a copy arrives with a flipped
    payload), damaged headers."""
    pr = lm.Params(seed=seed, first=0, window=window, flags=lm.DUP_FLIP if dup_flip else 0, dup=dup, bad_sym=bad_sym, foreign=foreign)
    src, fate = lm.plan(pr, pk.shape[0], None)
    return lm.apply(pk, src, fate)[0]


def random_stream(seed, nblocks=12, block0=0, S=S):
    """A stream that mixes what the rule distinguishes: loss per block from a few rates, reordering over up to about two blocks,
    duplicates with another payload, foreign block numbers, symbol numbers >= n."""
    rng = np.random.default_rng(seed)
    rates = rng.choice([1.0, 0.95, 0.9, 0.85, 0.7], size=nblocks)
    gap = int(rng.choice([0, 0, 3, 6]))   # an outage of whole blocks: what a re-anchor answers
    g0 = int(rng.integers(2, nblocks - 7))
    rates[g0:g0 + gap] = 0.0
    blk, sym = sent(nblocks, lambda b: rates[b], seed + 1, block0)
    return through_link(packets_of(blk, sym, S, seed=seed + 2), seed + 3, int(rng.choice([0, 30, 150, 400])), dup=0.03, bad_sym=0.01, foreign=0.02)


RANDOM_SEEDS = list(range(100, 112))
WRAP = dict(seed=200, nblocks=14, block0=248)   # block numbers 248 .. 255, 0 .. 5
WA = [(2, 0), (2, 10), (3, 10), (4, 10), (8, 3), (16, 10), (32, 1)]


def outage_stream():
    """40 blocks in order, 95 % kept, block 3 at 50 %."""
    return sent(40, lambda b: 0.5 if b == 3 else 0.95, 1)


def long_outage_stream():
    """40 blocks in order, 95 % kept, blocks 3 .. 20 lost entirely."""
    return sent(40, lambda b: 0.0 if 3 <= b <= 20 else 0.95, 1)


def reordered_stream():
    """60 blocks, 90 % kept, every packet delayed by 0 .. 1000 packet times (uniform): five blocks of reordering."""
    blk, sym = sent(60, lambda b: 0.9, 1)
    return through_link(packets_of(blk, sym, seed=5), 2, 1000)


# ---- the plan-edge stream of tests/test_gpu_rx_window.py: events placed on chosen lanes of the device scan's groups of 64 ----------
EDGE_W, EDGE_A = (2, 3, 16), (0, 10)


def edge_stream(A):
    """(blk, sym): full blocks 250 .. 255, 0 in order (closes by c == n, across the wrap), block 253 complete before block 252's packet
    km + 1 (two closes on adjacent packets), then one packet of block 1 and two runs of 11 packets 40 blocks ahead (with A = 10 a
    close by the ahead limit and a re-anchor, 11 packets apart; with A = 0 late packets), two more full blocks and a short tail.  A
    late packet and a bad symbol number in between."""
    blk, sym = [], []

    def add(b, syms):
        syms = list(syms)
        blk.extend([b & 0xFF] * len(syms))
        sym.extend(syms)

    add(250, range(N))
    add(245, [1])          # late
    add(251, range(N))
    add(251, [0xFFFF])     # bad symbol
    add(252, range(KM))    # c = km: no rule fires while block 253 fills
    add(253, range(N))
    add(252, [KM])         # c > km, later > 100 closes 252; 253 holds n packets already and closes at the packet after
    add(254, range(N))
    add(255, range(N))
    add(0, range(N))
    add(1, [3])
    add(41, range(11))
    add(41, range(11, 22))
    add(41, range(N))
    nb = 42 if A > 0 else 1
    add(nb, range(N))
    add(nb + 1, range(N))
    add(nb + 2, range(17))
    return np.array(blk, dtype=np.int64), np.array(sym, dtype=np.int64)


def edge_calls(blk, sym, W, A):
    """Call boundaries [(start, end)] that put the stream's events on lane 0, on lane 63 and on the last packet of a call, keep the
    pairs of events that are a few packets apart inside one group of 64, and end with a call of 17 packets."""
    ev = [p for p, _ in wm.events(blk, sym, N, K, W, A)]
    P = blk.shape[0]
    cuts = {ev[0] - 64, ev[1] - 63 - 64, ev[4] + 1, ev[5] - 20, P - 17}
    if A > 0:
        cuts.add(ev[8] - 30)   # the close by the ahead limit and the re-anchor behind it
    edges = [0] + sorted(cuts) + [P]
    return list(zip(edges[:-1], edges[1:]))


def edge_facts(blk, sym, W, A, calls):
    """What the calls place where, from the model alone: a set of tags."""
    ev = wm.events(blk, sym, N, K, W, A)
    facts = set()
    for s, e in calls:
        inside = [(p - s, kind) for p, kind in ev if s <= p < e]
        for q, kind in inside:
            facts.add("lane%d" % (q % 64) if q % 64 in (0, 63) else "mid")
            if s + q + 1 == e:
                facts.add("last packet of a call")
        groups = {}
        for q, kind in inside:
            groups.setdefault(q // 64, []).append(kind)
        for kinds in groups.values():
            if kinds.count("close") >= 2:
                facts.add("two closes in a group")
            if "close" in kinds and "resync" in kinds:
                facts.add("close and re-anchor in a group")
        if e - s < 64:
            facts.add("short call")
    return facts


def host_run(pk, W, A, max_blocks=1 << 20, cuts=()):
    """api.FecRxWindowHost over the stream, fed in the calls the cut positions make, each call repeated until it has consumed its
    piece: dict(blocks, sym, er, used (per call), stats, state)."""
    from ldpc_erasure_codes_amd import api
    S_ = pk.shape[1] - 8
    blocks, syms, ers, used = [], [np.zeros((0, N, S_), np.uint8)], [np.zeros((0, N), np.uint8)], []
    with api.FecRxWindowHost(N, K, S_, W, A) as rx:
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
        return dict(blocks=blocks, sym=np.concatenate(syms), er=np.concatenate(ers), used=used, stats=rx.stats(), state=rx.state(),
                    dropped=rx.dropped)


def model_run(pk, W, A):
    blk, sym = wm.headers(pk)
    return wm.run(blk, sym, N, K, W, A)
