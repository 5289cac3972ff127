"""numpy model of the link emulator (include/ldpc_erasure_amd_link.h, csrc/link_dev.hip), on ldpc_erasure_codes_amd/synth.py.

The model is the header's: packet i of a call has the entries e = 2i + c (c = 0 the original, c = 1 a copy), every draw is indexed by
g = first + i, an entry arrives at time i + c + delay(e) and the arrival order is the existing entries sorted by (time, e).

  draws(params, P, lost)             per-entry exists / delay / time / fate: pure functions of the index
  plan(params, P, lost)              the brute-force form: a stable sort on (time, e) -> (src int32 [Q], fate uint16 [Q])
  plan_windowed(params, P, lost, T)  the kernel's algorithm: tiles of T packets, a halo of window + 1 packets on either side,
                                     rank = prefix - (earlier entries that arrive later) + (later entries that arrive earlier)
  apply / apply_ragged               what the plan does to a packet array and to a trimmed wire
"""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldpc_erasure_codes_amd import synth  # noqa: E402

STREAM_DUP, STREAM_DELAY, STREAM_DAMAGE = 16, 17, 18
MAX_WINDOW = 4096
DUP_FLIP = 1
COPY, BADSYM, FOREIGN, FLIPPED = 1, 2, 4, 8
FEC_HEADER = 8
FLIP_BYTE = 0x5A
TILE = 256   # kTile of link_dev.hip

Params = collections.namedtuple("Params", "seed first window flags dup bad_sym foreign", defaults=(0, 0, 0, 0.0, 0.0, 0.0))
Draws = collections.namedtuple("Draws", "exists delay time fate")


def check(params, P):
    assert 0 <= P < 1 << 30
    assert 0 <= params.window <= MAX_WINDOW and (params.flags & ~DUP_FLIP) == 0
    assert all(0.0 <= p <= 1.0 for p in (params.dup, params.bad_sym, params.foreign)) and params.bad_sym + params.foreign <= 1.0


def draws(params, P, lost=None):
    """Per entry e = 2i + c, as [P][2] arrays: exists bool, delay int64, time int64 (relative to the call: i + c + delay), fate uint16."""
    check(params, P)
    i = np.arange(P, dtype=np.int64)
    with np.errstate(over="ignore"):
        g = np.uint64(params.first) + i.astype(np.uint64)
        idx = (g * np.uint64(2))[:, None] + np.arange(2, dtype=np.uint64)[None, :]
    alive = np.ones(P, dtype=bool) if lost is None else np.asarray(lost).reshape(P) == 0
    dup = synth.u32(params.seed, STREAM_DUP, g).astype(np.uint64) < np.uint64(synth.threshold(params.dup))
    exists = np.stack([alive, alive & dup], axis=1)
    delay = ((synth.u32(params.seed, STREAM_DELAY, idx).astype(np.uint64) * np.uint64(params.window + 1)) >> np.uint64(32)).astype(np.int64)
    time = i[:, None] + np.arange(2, dtype=np.int64)[None, :] + delay
    x = synth.u64(params.seed, STREAM_DAMAGE, idx)
    r = x >> np.uint64(32)
    t_bad = np.uint64(synth.threshold(params.bad_sym))
    t_for = np.uint64(synth.threshold(params.bad_sym) + synth.threshold(params.foreign))
    bad = r < t_bad
    foreign = ~bad & (r < t_for)
    fate = np.zeros((P, 2), dtype=np.uint16)
    fate[:, 1] |= COPY
    fate[bad] |= BADSYM
    fate[foreign] |= FOREIGN
    fate |= np.where(foreign, ((x >> np.uint64(8)) & np.uint64(0xFF)) << np.uint64(8), np.uint64(0)).astype(np.uint16)
    if params.flags & DUP_FLIP:
        fate[:, 1] |= FLIPPED
    return Draws(exists, delay, time, fate)


def plan(params, P, lost=None):
    """The arrival order by brute force: (src int32 [Q], fate uint16 [Q])."""
    d = draws(params, P, lost)
    e = np.nonzero(d.exists.reshape(-1))[0]
    order = e[np.argsort(d.time.reshape(-1)[e], kind="stable")]   # e ascends: a stable sort on time is the sort on (time, e)
    return (order >> 1).astype(np.int32), d.fate.reshape(-1)[order]


def ranks_windowed(params, P, lost=None, T=TILE):
    """rank int64 [P][2] (-1: the entry does not exist) and Q, the way link_plan_rank works them out: per tile of T packets the keys
    (0: no entry, else 1 + time - lo) of the tile and its halo, the tile bases from the per-tile counts, the in-tile scan, and
    for every owned entry the two counts over the packets within window + 1 of its own."""
    d = draws(params, P, lost)
    halo = params.window + 1
    ntiles = -(-P // T)
    counts = np.array([int(d.exists[t * T:(t + 1) * T].sum()) for t in range(ntiles)], dtype=np.int64)
    tilebase = np.concatenate([[0], np.cumsum(counts)])
    rank = np.full((P, 2), -1, dtype=np.int64)
    for t in range(ntiles):
        t0 = t * T
        lo, hi = max(0, t0 - halo), min(P, t0 + T + halo)
        keys = np.where(d.exists[lo:hi], 1 + d.time[lo:hi] - lo, 0).astype(np.uint32)   # [hi - lo][2]
        own = d.exists[t0:min(P, t0 + T)]
        per = own.sum(axis=1)
        excl = np.cumsum(per) - per
        for a in range(own.shape[0]):
            i = t0 + a
            if not own[a, 0]:
                continue
            base = int(tilebase[t] + excl[a])
            tA, tB = int(keys[i - lo, 0]), int(keys[i - lo, 1])
            left = keys[max(lo, i - halo) - lo:i - lo].reshape(-1)
            right = keys[i + 1 - lo:min(hi - 1, i + halo) + 1 - lo].reshape(-1)
            swap = int(tB != 0 and tB < tA)
            rank[i, 0] = base - int((left > tA).sum()) + int(((right != 0) & (right < tA)).sum()) + swap
            if tB:
                rank[i, 1] = base + 1 - int((left > tB).sum()) + int(((right != 0) & (right < tB)).sum()) - swap
    return rank, int(tilebase[-1])


def plan_windowed(params, P, lost=None, T=TILE):
    rank, Q = ranks_windowed(params, P, lost, T)
    d = draws(params, P, lost)
    src = np.full(Q, -1, dtype=np.int32)
    fate = np.zeros(Q, dtype=np.uint16)
    written = np.zeros(Q, dtype=np.int64)
    for c in (0, 1):
        i = np.nonzero(rank[:, c] >= 0)[0]
        np.add.at(written, rank[i, c], 1)
        src[rank[i, c]] = i
        fate[rank[i, c]] = d.fate[i, c]
    assert (written == 1).all(), "every position is written exactly once"
    return src, fate


def damage(packet, fate):
    """One packet (uint8 [>= 8]) under a fate word: a copy."""
    out = np.array(packet, dtype=np.uint8, copy=True)
    f = int(fate)
    if f & BADSYM:
        out[[0, 1, 4, 5]] = 0xFF
    if f & FOREIGN:
        out[[2, 6]] = f >> 8
    if f & FLIPPED:
        out[FEC_HEADER:] ^= FLIP_BYTE
    return out


def badsym_slot(plen):
    slot = np.zeros(plen, dtype=np.uint8)
    slot[[0, 1, 4, 5]] = 0xFF
    return slot


def apply(packets, src, fate, flow_of=None):
    """packets uint8 [P][8+S] -> (packets_out [Q][8+S], flow_of_out int32 [Q] or None).  A src outside 0 .. P-1: the BADSYM slot of
    zeros, flow -1."""
    packets = np.asarray(packets, dtype=np.uint8)
    P, plen = packets.shape
    Q = len(src)
    out = np.zeros((Q, plen), dtype=np.uint8)
    fo = None if flow_of is None else np.full(Q, -1, dtype=np.int32)
    for q in range(Q):
        s = int(src[q])
        if 0 <= s < P:
            out[q] = damage(packets[s], fate[q])
            if fo is not None:
                fo[q] = flow_of[s]
        else:
            out[q] = badsym_slot(plen)
    return out, fo


def ragged_lengths(offset, nbytes, src):
    """Length and start of every arriving datagram: land's vetting of the boundaries without the upper bound 8 + S."""
    offset = np.asarray(offset, dtype=np.int64)
    P = offset.shape[0] - 1
    ln = np.zeros(len(src), dtype=np.int64)
    start = np.zeros(len(src), dtype=np.int64)
    for q, s in enumerate(np.asarray(src, dtype=np.int64)):
        if not 0 <= s < P:
            continue
        o0, o1 = int(offset[s]), int(offset[s + 1])
        if 0 <= o0 <= o1 <= nbytes and o1 - o0 >= FEC_HEADER:
            ln[q], start[q] = o1 - o0, o0
    return ln, start


def apply_ragged(data, offset, src, fate, nbytes=None, bytes_cap=None):
    """data uint8 [nbytes], offset int64 [P+1] -> (bytes_out uint8 [total], offset_out int64 [Q+1]).  With bytes_cap, a datagram that
    would end beyond it is not written: its bytes are left 0 here (the device leaves them untouched) and lie beyond bytes_cap."""
    data = np.asarray(data, dtype=np.uint8)
    nbytes = data.shape[0] if nbytes is None else nbytes
    ln, start = ragged_lengths(offset, nbytes, src)
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    for q in range(len(src)):
        if ln[q] and (bytes_cap is None or off[q + 1] <= bytes_cap):
            out[off[q]:off[q + 1]] = damage(data[start[q]:start[q] + ln[q]], fate[q])
    return out, off
