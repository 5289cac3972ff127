"""Streams, call schedules and the host-side reference shared by tests/test_rxw_flows_cases_cpu.py and tests/test_gpu_rxw_flows.py
(numpy and the package's host side only): the windowed multi-flow receiver of include/ldpc_erasure_amd_rx_window_flows.h on
tests/rxw_cases.py's shapes.  The reference of every comparison is one api.FecRxWindowHost per flow (HostFlows)."""
import collections
import functools

import numpy as np

import rxw_cases as rc

wm = rc.wm
N, K, S = rc.N, rc.K, rc.S
SIZES = (0, 1, 17, 63, 64, 65, 300, 1111)   # packets a flow offers beyond its position, per call
MBS = (1, 2, 64)                            # max_blocks_per_flow of a call
LOCKSTEP_NFLOWS = (1, 3, 70)
LOCKSTEP_WA = [(2, 0), (4, 10), (32, 1)]


@functools.lru_cache(maxsize=None)
def _random_stream(seed, S_):
    pk = rc.random_stream(seed, S=S_)
    pk.setflags(write=False)
    return pk


@functools.lru_cache(maxsize=None)
def _wrap_stream(S_):
    pk = rc.random_stream(S=S_, **rc.WRAP)
    pk.setflags(write=False)
    return pk


def lockstep_streams(nflows, A):
    """One packet array per flow: flow f gets random_stream(RANDOM_SEEDS[f mod 12]); with more than one flow, flow 1 gets the WRAP
    stream (blocks 248 .. 255, 0 .. 5) and the last flow edge_stream(A); a single flow gets edge_stream(A)."""
    streams = [_random_stream(rc.RANDOM_SEEDS[f % len(rc.RANDOM_SEEDS)], S) for f in range(nflows)]
    if nflows > 1:
        streams[1] = _wrap_stream(S)
    streams[nflows - 1] = rc.packets_of(*rc.edge_stream(A))
    return streams


def concat(pieces, S_=S):
    """The per-flow pieces of one call as one segmented array: (packets uint8 [P][8 + S], flow_begin int64 [nflows + 1])."""
    fb = np.zeros(len(pieces) + 1, dtype=np.int64)
    fb[1:] = np.cumsum([p.shape[0] for p in pieces])
    pk = np.concatenate([np.asarray(p, dtype=np.uint8).reshape(-1, 8 + S_) for p in pieces]) if len(pieces) else np.zeros((0, 8 + S_), np.uint8)
    return np.ascontiguousarray(pk), fb


class HostFlows:
    """nflows api.FecRxWindowHost behind the multi-flow object's interface: the results in its layout, dense in flow (or list) order."""

    def __init__(self, nflows, W, A, S_=S, n=N, k=K):
        from ldpc_erasure_codes_amd import api
        self.nflows, self.n, self.S, self.W = nflows, n, S_, W
        self.rx = [api.FecRxWindowHost(n, k, S_, W, A) for _ in range(nflows)]

    def push_many(self, pieces, mb):
        """(closes int32 [nflows], blocks int32 [T], sym [T][n][S], er [T][n], consumed int64 [nflows]); an empty piece is no call."""
        closes, consumed = np.zeros(self.nflows, np.int32), np.zeros(self.nflows, np.int64)
        blocks, syms, ers = [], [np.zeros((0, self.n, self.S), np.uint8)], [np.zeros((0, self.n), np.uint8)]
        for f, (rx, piece) in enumerate(zip(self.rx, pieces)):
            if piece.shape[0] == 0:
                continue
            b, sy, er, u = rx.push_many(piece, mb)
            closes[f], consumed[f] = len(b), u
            blocks += b.tolist()
            syms.append(sy)
            ers.append(er)
        return closes, np.array(blocks, dtype=np.int32), np.concatenate(syms), np.concatenate(ers), consumed

    def flush_many(self, flows=None):
        """(closes int32 [nsel], blocks, sym, er) of FecRxWindowHost.flush() of every listed flow, dense in list order."""
        sel = list(range(self.nflows)) if flows is None else list(flows)
        closes, blocks = np.zeros(len(sel), np.int32), []
        syms, ers = [np.zeros((0, self.n, self.S), np.uint8)], [np.zeros((0, self.n), np.uint8)]
        for j, f in enumerate(sel):
            b, sy, er = self.rx[f].flush()
            closes[j] = len(b)
            blocks += b.tolist()
            syms.append(sy)
            ers.append(er)
        return closes, np.array(blocks, dtype=np.int32), np.concatenate(syms), np.concatenate(ers)

    def pending(self):
        """What a flush of every flow would hand out: blocks per flow (every open slot up to the last non-empty one)."""
        return [max([d + 1 for d, c in enumerate(rx.state()["cnt"]) if c > 0], default=0) for rx in self.rx]

    def stats(self, f):
        return self.rx[f].stats()

    def state(self, f):
        return self.rx[f].state()

    def dropped(self, f):
        return self.rx[f].dropped

    def close(self):
        for rx in self.rx:
            rx.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


Call = collections.namedtuple("Call", "mb spans pieces closes blocks sym er consumed")


def lockstep_calls(hx, streams, seed, sizes=SIZES, mbs=MBS):
    """The call schedule of the lockstep test, made while the host objects `hx` run it: per call every unfinished flow offers the
    packets from its position on, a random number of them from `sizes`, with a random max_blocks_per_flow from `mbs`; what a flow
    did not consume it offers again in the next call.  Yields Call(mb, spans [(start, end)] per flow, pieces, the host's results);
    hx holds the state after the call."""
    rng = np.random.default_rng(seed)
    nf = len(streams)
    pos = [0] * nf
    while any(pos[f] < streams[f].shape[0] for f in range(nf)):
        mb = int(rng.choice(mbs))
        take = rng.choice(sizes, size=nf)
        spans = [(pos[f], min(pos[f] + int(take[f]), streams[f].shape[0])) for f in range(nf)]
        pieces = [streams[f][a:b] for f, (a, b) in enumerate(spans)]
        closes, blocks, sym, er, consumed = hx.push_many(pieces, mb)
        for f in range(nf):
            pos[f] += int(consumed[f])
        yield Call(mb, spans, pieces, closes, blocks, sym, er, consumed)


def lockstep_seed(nflows, W, A):
    return 1000 * nflows + 10 * W + A


def count_ahead_closes(pk, W, A, n=N, k=K):
    """(closes by the ahead limit, re-anchors) over a whole stream, from the model: before each packet the counts are noted; a close
    after a packet whose slot-0 count c and later count fail `c == n or (c > kd and later > 10) or (c > km and later > 100)` can only
    be the ahead limit's."""
    blk, sym = wm.headers(pk)
    w = wm.Window(n, k, W, A)
    by_ahead = 0
    for b, s in zip(blk.tolist(), sym.tolist()):
        base = b if w.base == -1 else w.base
        cnt = list(w.cnt)
        d = (b - base) & 0xFF
        if s < n and d < W:
            cnt[d] += 1
        c, later = cnt[0], sum(cnt[1:])
        rule = c == n or (c > w.kd and later > 10) or (c > w.km and later > 100)
        if w.push(b, s) is not None and not rule:
            by_ahead += 1
    return by_ahead, w.totals["resyncs"]


# ---- the flush scenario: five flows, W = 4, A = 10 --------------------------------------------------------------------------------
FLUSH_W, FLUSH_A = 4, 10
FLUSH_LIST = [4, 1, 2, 0]   # non-ascending; flow 3 is not listed and goes on afterwards


def flush_streams(S_=S):
    """(before, after): the packets every flow gets before the flush, and those the flows get after it.  Flow 1 gets nothing (nothing
    open); flow 2 gets 50 packets of block 10 and 30 of block 12 (an empty slot between two non-empty ones); flows 0, 3, 4 get the
    first part of a stream, cut inside a block, and the rest after the flush."""
    r0, r3 = rc.random_stream(rc.RANDOM_SEEDS[4], S=S_), rc.random_stream(rc.RANDOM_SEEDS[5], S=S_)
    edge = rc.packets_of(*rc.edge_stream(FLUSH_A), S=S_)
    gap = rc.packets_of([10] * 50 + [12] * 30, list(range(50)) + list(range(30)), S=S_, seed=9)
    none = np.zeros((0, 8 + S_), np.uint8)
    before = [r0[:1500], none, gap, r3[:1300], edge[:900]]
    after = [r0[1500:], rc.random_stream(rc.RANDOM_SEEDS[6], S=S_)[:700], none, r3[1300:], edge[900:]]
    return before, after
