"""numpy model of the block-interleaved FEC wire (include/ldpc_erasure_amd_interleave.h): the order alone, a second statement of
ldpc_amd_fec_tx_ilv_layout beside the C one (csrc/wire_dev.hip).

  layout(nframes, n, block0, depth)   (first int64 [F], stride int32 [F]): row j of frame f is packet first[f] + j * stride[f]
  order(nframes, n, block0, depth)    (frame int64 [F n], row int64 [F n]) of every wire position
  headers(nframes, n, block0, depth)  (blk, sym) of the wire, what tools/rx_window_model.py takes
  interleave(packets, n, block0, depth)  straight-order packets [F n][..] -> wire order
  flows_order(frame_begin, n, block0, depth, order)  the multi-flow wire by brute force (include/ldpc_erasure_amd_interleave_flows.h)

depth D is 1, 2, 4, 8 or 16.  Frame f carries block (block0 + f) & 0xff and belongs to group block // D.  A run is a maximal set of
consecutive frames of one group, frames s .. s+m-1; it owns the packets n s .. n (s+m) - 1, and row j of its member i is packet
n s + j m + i.
"""
import numpy as np

DEPTHS = (1, 2, 4, 8, 16)


def layout(nframes, n, block0, depth):
    assert depth in DEPTHS and n >= 1 and nframes >= 0 and nframes * n < 2 ** 31
    f = np.arange(nframes, dtype=np.int64)
    group = ((block0 + f) & 0xFF) // depth
    # a run starts where the group changes (a group never follows itself: 256 / depth >= 16 groups lie between)
    start = np.ones(nframes, dtype=bool)
    start[1:] = group[1:] != group[:-1]
    run = np.cumsum(start) - 1
    s = np.flatnonzero(start)                                   # first frame of every run
    m = np.diff(np.append(s, nframes))                          # members of every run
    first = s[run] * n + (f - s[run])
    return first.astype(np.int64), m[run].astype(np.int32)


def order(nframes, n, block0, depth):
    first, stride = layout(nframes, n, block0, depth)
    pos = first[:, None] + np.arange(n, dtype=np.int64)[None, :] * stride[:, None]
    frame = np.empty(nframes * n, dtype=np.int64)
    row = np.empty(nframes * n, dtype=np.int64)
    frame[pos.ravel()] = np.repeat(np.arange(nframes, dtype=np.int64), n)
    row[pos.ravel()] = np.tile(np.arange(n, dtype=np.int64), nframes)
    return frame, row


def headers(nframes, n, block0, depth):
    frame, row = order(nframes, n, block0, depth)
    return (block0 + frame) & 0xFF, row


def interleave(packets, n, block0, depth):
    packets = np.asarray(packets)
    nframes = packets.shape[0] // n
    assert packets.shape[0] == nframes * n
    frame, row = order(nframes, n, block0, depth)
    return packets[frame * n + row]


SEGMENTED, ROUND_ROBIN = 0, 1


def flows_order(frame_begin, n, block0, depth, order_):
    """The multi-flow interleaved wire (include/ldpc_erasure_amd_interleave_flows.h) by brute force, no closed form: every flow's
    substream is order() of its own frames from its own block0, and a multiplexer merges the substreams -- SEGMENTED: one after the
    other; ROUND_ROBIN: round by round, in round q every flow that still has a q-th packet emits it, flows ascending, whatever the
    counts and block numbers are.  Returns (frame int64 [F n], row int64 [F n], flow int64 [F n]) of every wire position, `frame` a
    position in the source array (frame_begin[f] + the flow's own frame)."""
    fb = np.asarray(frame_begin, dtype=np.int64)
    nflows = fb.shape[0] - 1
    blk = np.broadcast_to(np.asarray(block0, dtype=np.int64) & 0xFF, (nflows,))
    subs = []
    for f in range(nflows):
        fr, row = order(int(fb[f + 1] - fb[f]), n, int(blk[f]), depth)
        subs.append((fr + fb[f], row))
    frame, row, flow = [], [], []
    if order_ == SEGMENTED:
        for f, (fr, rw) in enumerate(subs):
            frame += fr.tolist()
            row += rw.tolist()
            flow += [f] * fr.shape[0]
    else:
        assert order_ == ROUND_ROBIN
        for q in range(max([fr.shape[0] for fr, _ in subs], default=0)):
            for f, (fr, rw) in enumerate(subs):
                if q < fr.shape[0]:
                    frame.append(int(fr[q]))
                    row.append(int(rw[q]))
                    flow.append(f)
    return np.array(frame, dtype=np.int64), np.array(row, dtype=np.int64), np.array(flow, dtype=np.int64)
