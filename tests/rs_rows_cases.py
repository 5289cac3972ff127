"""Blocks shared by tests/test_rs_rows_cpu.py and tests/test_gpu_rs_rows.py (numpy, the oracle and the package's host side only): source
words, packets and staging rows for the Reed-Solomon decoder on rows in place (include/ldpc_erasure_amd_rs_rows.h).

The rows are random bytes, not codewords: the decoder solves for the message from the first k usable rows of a block whatever they
hold -- as ldpc_amd_rs_decode_frames and the oracle's decoder do -- so a test on random rows also shows that nothing else is read."""
import collections
import os
import sys

import numpy as np

import rs_wire_cases as rw

sys.path.insert(0, os.path.join(rw.rc.ROOT, "tools"))
import rs_rows_model as rr  # noqa: E402

rm = rw.rm
CODES = [(255, 192), (255, 223), (15, 11), (7, 3)]
EDGES = (0,) + rr.BUCKETS[:-1]   # r = edge and r = edge + 1 run different bodies of the stream kernel

# A block: kind[n] per symbol -- 'P' a packet of its own, 'S' a staging row of its own, 'E' erased, 'p' the packet index just past the
# array, 's' the staged row just past the array, 'D' the packet of the symbol before it
Case = collections.namedtuple("Case", "name kind")


def _kinds(n, erased, where, rng):
    """'E' at `erased`; the rest from packets ('P'), staging rows ('S') or both ('M': at least one of each)."""
    kind = np.array(["P" if where != "S" else "S"] * n)
    if where == "M":
        live = np.setdiff1d(np.arange(n), erased)
        if live.shape[0]:
            kind[rng.choice(live, size=max(1, live.shape[0] // 3), replace=False)] = "S"
    kind[np.asarray(erased, dtype=np.int64)] = "E"
    return kind


def cases(n, k, seed=0):
    """The blocks the issue names, for one code."""
    rng = np.random.default_rng(seed + 1000 * n + k)
    R = n - k
    rmax = min(R, k)   # a block misses at most this many source rows and is still decoded
    src_pos, rep_pos = np.arange(k), np.arange(k, n)
    out = []

    def add(name, erased, where="M"):
        out.append(Case(name, _kinds(n, np.asarray(erased, dtype=np.int64), where, rng)))

    add("complete", [])                                         # r = 0, more than k received
    add("first rmax source rows missing", np.concatenate([src_pos[:rmax], rep_pos[rmax:]]))   # exactly k, r = rmax (= R where R <= k)
    add("only repair rows missing", rep_pos)                    # exactly k, r = 0
    add("k - 1", rng.choice(n, size=R + 1, replace=False))      # short
    add("all erased", np.arange(n))
    add("packets only", rng.choice(src_pos, size=min(2, rmax), replace=False), "P")
    add("stage only", rng.choice(src_pos, size=min(2, rmax), replace=False), "S")
    for e in EDGES:                                             # one block at each bucket edge and one past it; more than k received where r < R
        for r in (e, e + 1):
            if 1 <= r <= rmax:
                lost_rep = rng.choice(rep_pos, size=int(rng.integers(0, R - r + 1)), replace=False)
                add("r = %d" % r, np.concatenate([rng.choice(src_pos, size=r, replace=False), lost_rep]))
    for b in rr.BUCKETS:                                        # one block inside each bucket
        lo = ([0] + list(rr.BUCKETS))[rr.BUCKETS.index(b)]
        r = min((lo + b + 1) // 2 + 1, rmax)
        if lo < r <= b:
            add("r = %d" % r, rng.choice(src_pos, size=r, replace=False))
    # k - 1 good rows and one word just past its array: taken as erased, the block is short
    for tag in "ps":
        erased = rng.choice(n, size=R + 1, replace=False)
        kind = _kinds(n, erased, "M", rng)
        kind[erased[0]] = tag
        out.append(Case("word past the %s" % ("packets" if tag == "p" else "staging rows"), kind))
    # two symbols of a block name one packet
    kind = _kinds(n, rng.choice(src_pos, size=min(2, rmax), replace=False), "P", rng)
    kind[k] = "D"   # (symbol k - 1 may be erased: then symbol k names the packet of the last live symbol before it)
    out.append(Case("one packet named twice", kind))
    return out


Built = collections.namedtuple("Built", "src packets stage first_k")


def build(cs, n, k, S, seed, garbage=0):
    """The words, the packet array and the staging rows of the blocks `cs`, rows handed out in a shuffled order.  garbage != 0: the rows
    behind the first k usable ones of every block hold other bytes; everything else is the same."""
    rng = np.random.default_rng(seed)
    B = len(cs)
    kinds = np.stack([c.kind for c in cs])
    nP, nS = int((kinds == "P").sum()), int((kinds == "S").sum())
    packets = rng.integers(0, 256, size=(nP, 8 + S), dtype=np.uint8)
    stage = rng.integers(0, 256, size=(nS, S), dtype=np.uint8)
    pid, sid = iter(rng.permutation(nP)), iter(rng.permutation(nS))
    src = np.full((B, n), rr.ROW_ERASED, dtype=np.uint32)
    first_k = np.zeros((B, n), dtype=bool)
    for b in range(B):
        last = None
        for j in range(n):
            c = kinds[b, j]
            if c == "P":
                src[b, j] = last = next(pid)
            elif c == "S":
                src[b, j] = rr.ROW_STAGED | next(sid)
            elif c == "p":
                src[b, j] = nP
            elif c == "s":
                src[b, j] = rr.ROW_STAGED | nS
            elif c == "D":
                assert last is not None
                src[b, j] = last
        pos, _ = rr.select(rr.vet(src[b], nP, nS), k)
        if pos is not None:
            first_k[b, pos] = True
    if garbage:
        g2 = np.random.default_rng(garbage)
        keep_p, keep_s = np.zeros(nP, dtype=bool), np.zeros(nS, dtype=bool)
        w = src[first_k].astype(np.int64)
        keep_p[w[(w & rr.ROW_STAGED) == 0]] = True
        keep_s[w[(w & rr.ROW_STAGED) != 0] & 0x7FFFFFFF] = True
        packets[~keep_p] = g2.integers(0, 256, size=(int((~keep_p).sum()), 8 + S), dtype=np.uint8)
        stage[~keep_s] = g2.integers(0, 256, size=(int((~keep_s).sum()), S), dtype=np.uint8)
    return Built(src, packets, stage, first_k)


def facts(cs, built, n, k):
    """What the blocks really hold, as tags."""
    out = set()
    nP, nS = built.packets.shape[0], built.stage.shape[0]
    for c, words in zip(cs, built.src):
        ok = rr.vet(words, nP, nS)
        cnt = int(ok.sum())
        w = words[ok].astype(np.int64)
        staged = (w & rr.ROW_STAGED) != 0
        if cnt:
            out.add("stage only" if staged.all() else "packets only" if not staged.any() else "mixed")
        if np.unique(w).shape[0] < w.shape[0]:
            out.add("one row named twice")
        past = [t for t, word in (("p", nP), ("s", rr.ROW_STAGED | nS)) if (words == word).any()]
        if cnt == 0:
            out.add("all erased")
        if cnt == k - 1:
            out.add("k - 1")
            out |= {"past the packets: short" if t == "p" else "past the staging rows: short" for t in past}
        if cnt < k:
            continue
        pos, _ = rr.select(ok, k)
        r = k - int((pos < k).sum())
        out |= {"r = %d" % r, "bucket %d" % rr.bucket(r)}
        if cnt > k:
            out.add("more than k")
        if cnt == k and r == min(n - k, k) and not ok[:r].any():
            out.add("exactly k, the first rmax source rows missing")
        if cnt == k and r == 0:
            out.add("exactly k, only repair rows missing")
    return out


def want(n, k):
    rmax = min(n - k, k)
    edges = {"r = %d" % r for e in EDGES for r in (e, e + 1) if r <= rmax}
    buckets = {"bucket %d" % rr.bucket(r) for r in range(rmax + 1)}
    return edges | buckets | {"r = %d" % rmax, "stage only", "packets only", "mixed", "one row named twice", "all erased", "k - 1", "more than k",
                              "past the packets: short", "past the staging rows: short", "exactly k, the first rmax source rows missing",
                              "exactly k, only repair rows missing"}


def reference(g, built):
    """rs_wire_model.decode_planes -- the oracle's decoder behind the first-k rule -- on the frames the words describe."""
    sym, er = rr.frames(built.src, built.packets, built.stage)
    return rm.decode_planes(g, sym, er) + (er,)
