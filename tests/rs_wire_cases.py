"""Streams and helpers shared by tests/test_rs_wire_cpu.py and tests/test_gpu_rs_wire.py (numpy, the oracle and the package's host side
only): Reed-Solomon blocks on the FEC wire of include/ldpc_erasure_amd_rs_wire.h."""
import os
import sys

import numpy as np

import interleave_cases as ic
import rxw_cases as rc

sys.path.insert(0, os.path.join(rc.ROOT, "tools"))
import rs_wire_model as rm  # noqa: E402
from oracle import oracle_py  # noqa: E402

wm, im = ic.wm, ic.im
S = 64
BLOCK0 = 250
WAD = [(2, 0, 1), (16, 10, 8), (32, 10, 16)]   # (window, ahead limit, depth)

_G = {}


def generator(n, k):
    if (n, k) not in _G:
        _G[n, k] = oracle_py.rs_generator(n, k)
    return _G[n, k]


def source(B, k, S_, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(B, k, S_), dtype=np.uint8)


def nblocks_for(D):
    """Blocks of the two pieces of a stream: the first more than two groups from BLOCK0 on, ending inside one; the second a group and a
    few blocks."""
    return max(2 * D + D // 2 + 3, 12), D + 3


def specials(D):
    """{block index: kind} of a two-piece stream.  The first piece holds a block that keeps exactly k symbols and behind it a complete
    one; the second ends with a complete block, one that is lost whole and one that keeps k - 1.  With a window of 2 and no ahead
    limit a block that cannot reach its threshold holds the window until a flush, and only a complete block closes in front of a lost
    one: there the special blocks end their pieces.  At a depth above 1 the first two sit in the first whole group, which lies inside
    the window from the first packet on: a forced close drops packets that are ahead of the window, and these blocks must lose none."""
    B1, B2 = nblocks_for(D)
    g = B1 - 3 if D == 1 else (D - BLOCK0 % D) % D
    return {g + 1: "k", g + 2: "full", B1 + B2 - 3: "full", B1 + B2 - 2: "lost", B1 + B2 - 1: "k-1"}


def arrive(pk, n, k, special, seed):
    """Wire packets through tools/link_model.py's link -- reordering within a few packets, duplicates carrying another payload, foreign
    block numbers, symbol numbers >= n -- then thinned by header: a block named in `special` ({block number: kind}) keeps exactly k
    or k - 1 distinct symbols, or nothing, or arrives whole and undamaged in one run; every other block loses 0, 2 or 5 % of what
    arrived, which leaves it above the receiver's lower threshold."""
    rng = np.random.default_rng(seed)
    a = rc.through_link(pk, seed + 1, 6, dup=0.03, bad_sym=0.01, foreign=0.02)
    blk, sym = wm.headers(a)
    # (a foreign number just behind the piece's last block would sit in the window at the flush, which hands out every slot up to the
    # last one that holds a packet: the next piece would then start behind the window's base.  Those few packets go.)
    end = int(wm.headers(pk)[0][-1])
    a = a[((blk - end - 1) & 0xFF) >= 32]
    blk, sym = wm.headers(a)
    keep = np.ones(a.shape[0], dtype=bool)
    splice = {}
    for b in np.unique(blk):
        idx = np.flatnonzero(blk == b)
        kind = special.get(int(b))
        if kind == "lost":
            keep[idx] = False
        elif kind in ("k", "k-1"):
            have = np.unique(sym[idx][sym[idx] < n])
            chosen = rng.choice(have, size=k if kind == "k" else k - 1, replace=False)
            keep[idx] = np.isin(sym[idx], chosen)
        elif kind == "full":
            keep[idx] = False
            splice[int(idx[idx.shape[0] // 2])] = pk[wm.headers(pk)[0] == b]   # (the median: a foreign packet may carry the number early)
        else:
            keep[idx] = rng.random(idx.shape[0]) < rng.choice([1.0, 0.98, 0.95])
    out, last = [], 0
    for pos in sorted(splice):
        out += [a[last:pos][keep[last:pos]], splice[pos]]
        last = pos
    out.append(a[last:][keep[last:]])
    return np.concatenate(out)


def pieces(wire, n, k, D, seed):
    """The two arrived pieces of a stream; wire(first block index, count, block number of the first) -> the sender's packets."""
    B1, B2 = nblocks_for(D)
    sp = [{(BLOCK0 + j) & 0xFF: kind for j, kind in specials(D).items() if (j >= B1) == second} for second in (False, True)]
    return [arrive(wire(0, B1, BLOCK0), n, k, sp[0], seed), arrive(wire(B1, B2, (BLOCK0 + B1) & 0xFF), n, k, sp[1], seed + 7)]


def model_blocks(parts, n, k, W, A, D):
    """What the receiver's rule hands out over the pieces, each followed by a flush: [(closed by the piece, closed by its flush)],
    lists of (number, {symbol: index into the piece}); every flush is a forced close."""
    w = wm.Window(n, k, W, A, D)
    out = []
    for pk in parts:
        blk, sym = wm.headers(pk)
        seen = w.seen
        closed, used = w.push_many(blk, sym, 1 << 30)
        assert used == pk.shape[0]
        out.append(([(b, {s: p - seen for s, p in win.items()}) for b, win in closed],
                    [(b, {s: p - seen for s, p in win.items()}) for b, win in w.flush()]))
    return out


def facts(handed, n, k):
    """What a receiver handed out, as tags; handed: lists of (number, {symbol: packet index}) of the model."""
    out = set()
    for number, win in handed:
        c = len(win)
        out |= {"exactly k"} if c == k else {"k - 1"} if c == k - 1 else {"complete"} if c == n else {"all-erased"} if c == 0 else set()
    return out


WANT = {"exactly k", "k - 1", "complete", "all-erased"}


def host_reference(decode, parts, n, k, W, A, D, cuts, max_blocks):
    """api.FecRxWindowHost over the pieces, every piece cut into calls at cuts[piece] and flushed; a call that stops early is followed
    by calls over the rest of its piece.  decode(sym, er) -> what the test compares.  Returns [(calls of the piece, its flush)], a call
    = dict(blocks, dec, er, used, stats, state)."""
    from ldpc_erasure_codes_amd import api
    out = []
    with api.FecRxWindowHost(n, k, parts[0].shape[1] - 8, W, A, depth=D) as rx:
        for pk, cut in zip(parts, cuts):
            calls = []
            edges = [0] + list(cut) + [pk.shape[0]]
            for s, e in zip(edges[:-1], edges[1:]):
                pos = s
                while pos < e:
                    bl, sy, er, used = rx.push_many(pk[pos:e], max_blocks)
                    calls.append(dict(blocks=bl.tolist(), dec=decode(sy, er), er=er, used=used, stats=rx.stats(), state=rx.state()))
                    pos += used
            fb, fs, fe = rx.flush()
            out.append((calls, dict(blocks=fb.tolist(), dec=decode(fs, fe), er=fe, stats=rx.stats(), state=rx.state())))
    return out
