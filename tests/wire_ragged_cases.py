"""Inputs and a scalar restatement of land shared by tests/test_wire_ragged_cpu.py and tests/test_gpu_wire_ragged.py (numpy and the
package's host side only)."""
import os
import sys

import numpy as np

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import datagram_frames as dg  # noqa: E402

FAR = 1 << 62


def edge_lengths(rng, N, S, p_special=0.5):
    """Datagram lengths: the edge lengths 0, 1, 2, 3, 4, 5, S - 5, S - 4 (where S admits them) mixed with random ones."""
    pool = [v for v in (0, 1, 2, 3, 4, 5, S - 5, S - 4) if 0 <= v <= S - 4]
    return np.array([int(rng.choice(pool)) if rng.random() < p_special else int(rng.integers(0, S - 3)) for _ in range(N)], dtype=np.int64)


def pack_made_frames(rng, F, n, k, S, short=0):
    """(frames uint8 [F][n][S], datagram offsets): source rows made by the datagram model's pack from datagrams of edge_lengths (the
    last `short` rows are the fillers pack adds), repair rows noise."""
    N = F * k - short
    ln = edge_lengths(rng, N, S)
    off = np.concatenate([[3], 3 + np.cumsum(ln)]).astype(np.int64)
    data = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    frames = rng.integers(0, 256, size=(F, n, S), dtype=np.uint8)
    frames[:, :k] = dg.pack(data, off, k, S)
    return frames, off


def host_packets(rng, F, n, k, S, short=0, block0=254):
    """(packets uint8 [F*n][8+S], datagram offsets) through the host packetiser."""
    frames, off = pack_made_frames(rng, F, n, k, S, short)
    return api.fec_packetize(frames, fec_class=1, block0=block0), off


def plant_bad(o, nbytes, S, at=(3, 8, 12)):
    """A copy of the offsets o (at least 14 datagrams) with a datagram of every REJECTED kind planted; returns (offsets, {kind: index}).
    Rewriting entry p + 1 moves the end of datagram p AND the start of datagram p + 1: the neighbour lands other bytes or is rejected
    in its turn, which land_scalar below states.  Datagram 0 is left alone."""
    a, b, c = at
    o = np.concatenate([o, [o[-1] + 7, o[-1] + 7 + 8 + S + 1]]).astype(np.int64)   # two more datagrams: 7 bytes, and 8 + S + 1
    P = o.shape[0] - 1
    kinds = {"len 7": P - 2, "len 8 + S + 1": P - 1}
    o[a + 1] = o[a] - 5                  # datagram a ends before it begins
    kinds["decreasing"] = a
    o[b] = -9                            # datagram b starts below 0 (datagram b - 1 ends there)
    kinds["negative"], kinds["decreasing to a negative"] = b, b - 1
    o[c + 1] = nbytes + 100              # datagram c ends beyond the buffer (datagram c + 1 starts there)
    kinds["end beyond nbytes"], kinds["start beyond nbytes"] = c, c + 1
    return o, kinds


def plant_far(o, at=(16, 20)):
    """... and offsets that point far outside any buffer: FAR and -FAR, whose differences do not fit 64 bits."""
    a, b = at
    o = o.copy()
    o[a], o[a + 1] = FAR, -FAR
    o[b], o[b + 1] = -FAR, FAR
    return o, {"far end": a - 1, "far decreasing": a, "far negative": a + 1, "far negative end": b - 1, "far span": b, "far start": b + 1}


def land_scalar(data, o, nbytes, S):
    """Land, one datagram at a time in Python integers: (packets [P][8+S], state [P])."""
    P = len(o) - 1
    packets = np.zeros((P, 8 + S), dtype=np.uint8)
    state = np.zeros(P, dtype=np.uint8)
    for p in range(P):
        a, b = int(o[p]), int(o[p + 1])
        if 0 <= a <= b <= nbytes and 8 <= b - a <= 8 + S:
            packets[p, :b - a] = data[a:b]
        else:
            packets[p, :8] = 0xFF
            state[p] = 1
    return packets, state
