"""Interleaving for the mixed calls of the multi-flow receiver (include/ldpc_erasure_amd_flows_mixed.h), on the host alone: turns the
per-flow segments of one call (flow_streams.call_packets' inputs) into ONE packet array in an arrival order plus flow_of, the flow
number of every packet.  Every pattern preserves each flow's own order, so de-interleaving with a stable sort by flow gives the
segments back.

Patterns (PATTERNS):
  random       a uniformly random merge
  round_robin  strict round robin over the flows that still have packets: with 64 or more such flows every lane of a group of 64
               holds a different flow
  runs         the flows take turns with runs of `run` packets (more than 64, and more than a tile of the partition)
  single       flow by flow in ascending order, each flow one run: with one non-empty flow the call is that flow only
  reverse      flow by flow in descending order
Each comes with and without unrouted packets (flow numbers -1, nflows and 2^31 - 1) sprinkled in; their payload is noise.

This module imports nothing of the code under test: numpy only."""
import numpy as np

PATTERNS = ("random", "round_robin", "runs", "single", "reverse")
RUN = 1100          # "runs": above the partition's smallest tile of 1024 packets
UNROUTED = (-1, None, 2**31 - 1)   # None stands for nflows


def flow_ids(lens, pattern, rng, run=RUN):
    """int32 [sum(lens)]: the flow of every position of the interleaved array, flow f appearing lens[f] times.  (The r-th
    appearance of f is the r-th packet of flow f: the order inside a flow is kept by construction.)"""
    lens = np.asarray(lens, dtype=np.int64)
    flow = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    rank = np.concatenate([np.arange(c, dtype=np.int64) for c in lens]) if lens.size else np.zeros(0, np.int64)
    if pattern == "random":
        ids = flow[rng.permutation(flow.size)]
    elif pattern == "round_robin":
        ids = flow[np.lexsort((flow, rank))]            # by rank, then flow
    elif pattern == "runs":
        ids = flow[np.lexsort((rank, flow, rank // run))]
    elif pattern == "single":
        ids = flow
    elif pattern == "reverse":
        ids = flow[np.lexsort((rank, -flow))]
    else:
        raise KeyError(pattern)
    return ids.astype(np.int32)


def sprinkle(ids, nflows, rng, frac=0.1):
    """ids with unrouted flow numbers inserted at random places: at least one of each of -1, nflows and 2^31 - 1."""
    vals = np.array([nflows if v is None else v for v in UNROUTED], dtype=np.int64)
    U = max(len(vals), int(ids.size * frac))
    extra = np.concatenate([vals, vals[rng.integers(0, len(vals), size=U - len(vals))]])
    at = np.sort(rng.integers(0, ids.size + 1, size=U))
    return np.insert(ids.astype(np.int64), at, extra[rng.permutation(U)]).astype(np.int32)


def flow_of_for(lens, pattern, seed, unrouted=False, run=RUN):
    """flow_of int32 [P] for per-flow packet counts `lens` (nflows = len(lens))."""
    rng = np.random.default_rng(seed)
    ids = flow_ids(lens, pattern, rng, run)
    return sprinkle(ids, len(lens), rng) if unrouted else ids


def mix(segments, pattern, seed, unrouted=False, run=RUN):
    """(packets uint8 [P][plen], flow_of int32 [P]) of one call: `segments` (one uint8 [c_f][plen] array per flow) interleaved."""
    nflows = len(segments)
    plen = segments[0].shape[1]
    flow_of = flow_of_for([s.shape[0] for s in segments], pattern, seed, unrouted, run)
    packets = np.random.default_rng(seed + 1).integers(0, 256, size=(flow_of.size, plen), dtype=np.uint8)   # noise where no flow's packet goes
    for f, s in enumerate(segments):
        packets[flow_of == f] = s
    return np.ascontiguousarray(packets), flow_of


def demux(flow_of, nflows):
    """The reference partition: (order int64 [R], counts int64 [nflows], flow_begin int64 [nflows + 1])."""
    routed = (flow_of >= 0) & (flow_of < nflows)
    idx = np.flatnonzero(routed)
    order = idx[np.argsort(flow_of[idx], kind="stable")]
    counts = np.bincount(flow_of[idx], minlength=nflows).astype(np.int64)
    return order, counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def left_model(flow_of, nflows, used):
    """left uint8 [P]: 1 for a routed packet whose rank in its flow is >= used[flow]."""
    left = np.zeros(flow_of.size, dtype=np.uint8)
    for f in range(nflows):
        at = np.flatnonzero(flow_of == f)
        left[at[int(used[f]):]] = 1
    return left
