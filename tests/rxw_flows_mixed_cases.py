"""Interleaved calls shared by tests/test_rxw_flows_mixed_cases_cpu.py and tests/test_gpu_rxw_flows_mixed.py (numpy only): the
lockstep schedule of tests/rxw_flows_cases.py with every call's per-flow pieces merged into ONE packet array in an arrival order plus
flow_of, by tools/flow_mix.py.  The pattern and whether unrouted packets are sprinkled in follow from the call's number alone."""
import numpy as np

import rxw_flows_cases as fc   # (puts tools/ on the path)

import flow_mix as fm  # noqa: E402

SHORT_RUN = 70   # "runs" in a short call: still more than a group of 64 lanes


def mix_seed(seed, i):
    return 100 * seed + i


def mixed_call(call, i, seed):
    """(packets uint8 [P][8 + S], flow_of int32 [P]) of call number i of a lockstep schedule made with `seed`: pattern
    PATTERNS[i % 5], unrouted packets in the odd calls.  "runs" takes turns of fm.RUN packets (more than a partition tile) where the
    call is long enough for every turn to be a full one for some flows, else of SHORT_RUN."""
    total = sum(p.shape[0] for p in call.pieces)
    run = fm.RUN if total >= 3 * fm.RUN else SHORT_RUN
    return fm.mix(call.pieces, fm.PATTERNS[i % len(fm.PATTERNS)], mix_seed(seed, i), unrouted=bool(i & 1), run=run)


def unrouted_in(flow_of, nflows):
    return int(((flow_of < 0) | (flow_of >= nflows)).sum())


def deinterleave(packets, flow_of, nflows):
    """(packets of seg_0 | seg_1 | ..., flow_begin) by numpy's stable sort: the array the segmented call takes."""
    order, _, fb = fm.demux(flow_of, nflows)
    return np.ascontiguousarray(packets[order]), fb
