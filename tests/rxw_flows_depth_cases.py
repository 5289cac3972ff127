"""Streams and the host-side reference shared by tests/test_rxw_flows_depth_cases_cpu.py and tests/test_gpu_rxw_flows_depth.py (numpy
and the package's host side only): the windowed multi-flow receiver created with a depth (include/ldpc_erasure_amd_interleave_flows.h)
on tests/rxw_cases.py's shape n = 200, k = 150, S = 16.  The per-flow streams are tests/interleave_cases.py's, the call schedules
tests/rxw_flows_cases.py's, and the reference of every comparison is one api.FecRxWindowHost(depth = D) per flow (HostFlowsDepth)."""
import functools

import numpy as np

import interleave_cases as ic
import rxw_cases as rc
import rxw_flows_cases as fc

wm = rc.wm
N, K, S = rc.N, rc.K, rc.S
LOCKSTEP_NFLOWS = (1, 3, 70)
LOCKSTEP_WD = [(4, 2), (9, 4), (16, 8), (32, 16), (32, 4)]
AHEAD = (0, 10)
LINK_WINDOWS = (0, 64)


class HostFlowsDepth(fc.HostFlows):
    """fc.HostFlows of api.FecRxWindowHost(..., depth = D) objects."""

    def __init__(self, nflows, W, A, D, S_=S, n=N, k=K):
        from ldpc_erasure_codes_amd import api
        self.nflows, self.n, self.S, self.W, self.D = nflows, n, S_, W, D
        self.rx = [api.FecRxWindowHost(n, k, S_, W, A, depth=D) for _ in range(nflows)]
        assert all(rx.depth == D for rx in self.rx)


@functools.lru_cache(maxsize=None)
def _stream(seed, D, block0, link_window):
    pk = ic.stream(seed, D, block0, link_window)
    pk.setflags(write=False)
    return pk


@functools.lru_cache(maxsize=None)
def _edge():
    pk = rc.packets_of(*ic.edge_stream())
    pk.setflags(write=False)
    return pk


def stream_args(f, D):
    """(seed, D, block0, link_window) of flow f's stream: another seed per flow, block0 alternating 248 and 250, the link's reorder
    window alternating 0 and 64 at half that pace.  A seed whose stream opens with a packet the link gave a foreign block number is
    passed over (the next candidate is 5000 on): the window would anchor far from the stream and both the plain and the depth-D rule
    drop all of it as late, which shows nothing about the depth."""
    block0, link_window = ic.BLOCK0[f % 2], LINK_WINDOWS[(f // 2) % 2]
    seed = 7001 + 100 * D + f
    while ((int(wm.headers(_stream(seed, D, block0, link_window)[:1])[0][0]) - (block0 - block0 % D)) & 0xFF) >= D:
        seed += 5000
    return seed, D, block0, link_window


def empty_flow(nflows):
    """The flow that gets nothing (none when there is only one)."""
    return 1 if nflows > 2 else None


def edge_flow(nflows, W, D, A):
    """The flow that gets interleave_cases.edge_stream(), where the stream's depth and window are the object's: the last one.  A
    single flow gets it only without an ahead limit, where the blocks of its own stream -- 248 or 250 is no multiple of 16 -- never
    close; with one it keeps its own stream, the one with the forced closes."""
    if (W, D) != (ic.EDGE_W, ic.EDGE_D) or (nflows == 1 and A > 0):
        return None
    return nflows - 1


def lockstep_streams(nflows, W, D, A):
    """One packet array per flow: interleave_cases.stream with stream_args(f, D); one flow gets nothing; at D = 16, W = 32 the flow
    edge_flow names gets the plan-edge stream (the g == 1 close across the 8-bit wrap, the re-anchor into slot 5)."""
    streams = [_stream(*stream_args(f, D)) for f in range(nflows)]
    if empty_flow(nflows) is not None:
        streams[empty_flow(nflows)] = np.zeros((0, 8 + S), np.uint8)
    if edge_flow(nflows, W, D, A) is not None:
        streams[edge_flow(nflows, W, D, A)] = _edge()
    return streams


def lockstep_seed(nflows, W, A, D):
    return 100000 * D + fc.lockstep_seed(nflows, W, A)


def stream_facts(pk, W, A, D):
    """What a stream holds under the depth-D rule, from the model alone (tools/rx_window_model.py): a set of tags."""
    return _stream_facts(pk.tobytes(), pk.shape[1], W, A, D)


@functools.lru_cache(maxsize=None)
def _stream_facts(raw, plen, W, A, D):
    blk, sym = wm.headers(np.frombuffer(raw, dtype=np.uint8).reshape(-1, plen))
    facts = set()
    if blk.shape[0] == 0:
        return facts
    w = wm.Window(N, K, W, A, D)
    for b, s in zip(blk.tolist(), sym.tolist()):
        base = b - b % D if w.base == -1 else w.base
        cnt = list(w.cnt)
        d = (b - base) & 0xFF
        if s < N and d < W:
            cnt[d] += 1
        g = D - base % D
        c, later = cnt[0], sum(cnt[g:])
        rule = c == N or (c > w.kd and later > 10) or (c > w.km and later > 100)
        resyncs = w.totals["resyncs"]
        closed = w.push(b, s) is not None
        if closed and not rule:
            facts.add("forced close")
        if closed and g == 1:
            facts.add("g == 1 close")
        if w.totals["resyncs"] > resyncs and b % D != 0:   # the window starts at the group, below the block of the tripping packet
            facts.add("re-anchor below the first block seen")
    plain = wm.Window(N, K, W, A, 1)
    closed1, _ = plain.push_many(blk, sym, 1 << 30)
    deep = wm.Window(N, K, W, A, D)
    closedD, _ = deep.push_many(blk, sym, 1 << 30)
    if [c[0] for c in closed1] != [c[0] for c in closedD] or plain.totals["late"] != deep.totals["late"]:
        facts.add("the plain rule differs")
    return facts


WANT = {"forced close", "re-anchor below the first block seen", "g == 1 close"}
