"""numpy model of the windowed FEC receiver (include/ldpc_erasure_amd_rx_window.h), on (block, symbol) arrays alone: a third
statement of the rule beside the C host object (csrc/rx_window.cpp) and the device scan (csrc/rx_window_dev.hip).  No payloads: a
closed block is the list of the packet indices that won its symbols (the last copy of a symbol wins).

  headers(packets)                         (blk, sym) int arrays of a packet array uint8 [P][8 + S]
  Window(n, k, W, A, D=1, rule=None)       the state; .push_many(blk, sym, max_blocks) -> (closed, consumed); .flush() -> closed
  run(blk, sym, n, k, W, A, max_blocks, D, rule)  one call over a whole stream: Result(closed, consumed, totals, state)
  two_buffer(blk, sym, n, k)               the reference draft's two-buffer rule (csrc/wire.cpp), for comparison
  events(blk, sym, n, k, W, A, D=1, rule=None)  the packet indices after which the model closed or re-anchored
  default_rule(n, k), mds_rule(n, k, D=1, giveup=0)  the presets of include/ldpc_erasure_amd_rx_rule.h

rule is the close rule as a value, (c_hi, later_hi, c_lo, later_lo): slot 0 closes when c == n, c >= c_hi and later >= later_hi, or
c >= c_lo and later >= later_lo.  None means default_rule(n, k), the rule the receiver always had.

D is the interleaving depth of include/ldpc_erasure_amd_interleave.h: blocks b with equal b // D form a group, the window anchors on
group starts, and `later` of the close test counts the slots of later groups only.  D = 1 is the plain rule.

closed: a list of (block number, {symbol: winning packet index}); packet indices count from the start of the stream the Window has
seen (its .seen counter), so results of split calls compare with those of one call.
"""
import collections

import numpy as np

TOTALS = ("bad_symbol", "late", "ahead_total", "resyncs", "closed")
Result = collections.namedtuple("Result", "closed consumed totals state")


def headers(packets):
    packets = np.asarray(packets, dtype=np.uint8)
    return packets[:, 2].astype(np.int64), packets[:, 0].astype(np.int64) | (packets[:, 1].astype(np.int64) << 8)


def thresholds(n, k):
    """(kd, km) = (k + round(0.8 (n-k)), k + round(0.2 (n-k))), rounding half away from zero as C's lround does."""
    return k + int(np.floor((n - k) * 0.8 + 0.5)), k + int(np.floor((n - k) * 0.2 + 0.5))


def default_rule(n, k):
    """(kd + 1, 11, km + 1, 101): `c > kd and later > 10 or c > km and later > 100` on integers."""
    kd, km = thresholds(n, k)
    return (min(kd + 1, n), 11, km + 1, 101)   # n - k <= 2: kd = n, and `c >= n` adds nothing to the rule's own c == n


def mds_rule(n, k, D=1, giveup=0):
    """(k, 1, 0, giveup) for a code that decodes from any k symbols on a wire that is roughly in order; giveup == 0: max(1, D k // 2)."""
    return (k, 1, 0, giveup if giveup else max(1, D * k // 2))


def rule_ok(n, rule):
    """The validity condition of include/ldpc_erasure_amd_rx_rule.h."""
    c_hi, l_hi, c_lo, l_lo = rule
    return all(0 <= c <= n and 0 <= l <= 1 << 30 and (c > 0 or l >= 1) for c, l in ((c_hi, l_hi), (c_lo, l_lo)))


class Window:
    def __init__(self, n, k, W, A, D=1, rule=None):
        assert 2 <= W <= 32 and A >= 0
        assert D in (1, 2, 4, 8, 16) and (D == 1 or 2 * D <= W)
        self.n, self.k, self.W, self.A, self.D = n, k, W, A, D
        self.kd, self.km = thresholds(n, k)
        self.rule = tuple(int(v) for v in rule) if rule is not None else default_rule(n, k)
        assert len(self.rule) == 4 and rule_ok(n, self.rule)
        self.base, self.ahead, self.seen = -1, 0, 0
        self.cnt = [0] * W
        self.slots = [dict() for _ in range(W)]
        self.totals = dict.fromkeys(TOTALS, 0)
        self.events = []   # (packet index, "close" | "resync")
        self.event_base = []   # base when the event fired, one entry per event
        # one entry per event: "full" (c == n), "hi" / "lo" (the clause of the rule that held; "hi" where both did), "ahead" (the
        # forced close by the ahead limit), "resync"; and the count of slot 0 at that moment
        self.event_why, self.event_c = [], []

    def state(self):
        return dict(base=self.base, cnt=list(self.cnt), ahead=self.ahead)

    def _close(self):
        out = (self.base, self.slots.pop(0))
        self.slots.append(dict())
        self.cnt = self.cnt[1:] + [0]
        self.base = (self.base + 1) & 0xFF
        self.ahead = 0
        self.totals["closed"] += 1
        return out

    def push(self, blk, sym):
        """One packet: the closed block or None."""
        p = self.seen
        self.seen += 1
        if self.base == -1:
            self.base = blk - blk % self.D
        if sym >= self.n:
            self.totals["bad_symbol"] += 1
        else:
            d = (blk - self.base) & 0xFF
            if d < self.W:
                self.slots[d][sym] = p
                self.cnt[d] += 1
            elif self.A > 0 and d < 128:
                self.ahead += 1
                self.totals["ahead_total"] += 1
            else:
                self.totals["late"] += 1
        g = self.D - self.base % self.D   # open slots of slot 0's group
        c, later, rest = self.cnt[0], sum(self.cnt[g:]), sum(self.cnt)
        c_hi, l_hi, c_lo, l_lo = self.rule
        if c == self.n or (c >= c_hi and later >= l_hi) or (c >= c_lo and later >= l_lo):
            self.events.append((p, "close"))
            self.event_base.append(self.base)
            self.event_why.append("full" if c == self.n else "hi" if c >= c_hi and later >= l_hi else "lo")
            self.event_c.append(c)
            return self._close()
        if self.A > 0 and self.ahead > self.A:
            if rest == 0:
                self.base = blk - blk % self.D
                self.slots[blk % self.D][sym] = p
                self.cnt[blk % self.D] = 1
                self.ahead = 0
                self.totals["resyncs"] += 1
                self.events.append((p, "resync"))
                self.event_base.append(self.base)
                self.event_why.append("resync")
                self.event_c.append(0)
                return None
            self.events.append((p, "close"))
            self.event_base.append(self.base)
            self.event_why.append("ahead")
            self.event_c.append(c)
            return self._close()
        return None

    def push_many(self, blk, sym, max_blocks):
        closed, i = [], 0
        while i < len(blk) and len(closed) < max_blocks:
            r = self.push(int(blk[i]), int(sym[i]))
            i += 1
            if r is not None:
                closed.append(r)
        return closed, i

    def flush(self):
        count = max([d + 1 for d in range(self.W) if self.cnt[d] > 0], default=0)
        return [self._close() for _ in range(count)]


def run(blk, sym, n, k, W, A, max_blocks=1 << 30, D=1, rule=None):
    w = Window(n, k, W, A, D, rule)
    closed, used = w.push_many(blk, sym, max_blocks)
    return Result(closed, used, dict(w.totals), w.state())


def events(blk, sym, n, k, W, A, D=1, rule=None):
    w = Window(n, k, W, A, D, rule)
    w.push_many(blk, sym, 1 << 30)
    return list(w.events)


def two_buffer(blk, sym, n, k):
    """The draft's rule as csrc/wire.cpp restates it: (closed [(block, {symbol: packet})], dropped).  Written out on its own, not as
    Window(W = 2, A = 0), so that the anchor is a comparison of two statements."""
    kd, km = thresholds(n, k)
    cur = nxt = -1
    ccnt = ncnt = dropped = 0
    bufs = [dict(), dict()]
    closed = []
    for p in range(len(blk)):
        b, s = int(blk[p]), int(sym[p])
        if cur == -1 and nxt == -1:
            cur, nxt = b, (b + 1) & 0xFF
        if s >= n:
            dropped += 1
        elif b == cur:
            bufs[0][s] = p
            ccnt += 1
        elif b == nxt:
            bufs[1][s] = p
            ncnt += 1
        else:
            dropped += 1
        if ccnt == n or (ccnt > kd and ncnt > 10) or (ccnt > km and ncnt > 100):
            closed.append((cur, bufs[0]))
            bufs = [bufs[1], dict()]
            cur, nxt, ccnt, ncnt = nxt, (nxt + 1) & 0xFF, ncnt, 0
    return closed, dropped


def rows(closed):
    """Distinct symbols per closed block."""
    return [len(s) for _, s in closed]


def planes(closed, packets, n):
    """The bytes the model implies: (blocks int32 [B], sym uint8 [B][n][S], erased uint8 [B][n]) for winning indices into `packets`."""
    packets = np.asarray(packets, dtype=np.uint8)
    S = packets.shape[1] - 8
    B = len(closed)
    sym = np.zeros((B, n, S), dtype=np.uint8)
    er = np.ones((B, n), dtype=np.uint8)
    for j, (_, win) in enumerate(closed):
        for s, p in win.items():
            sym[j, s] = packets[p, 8:]
            er[j, s] = 0
    return np.array([b for b, _ in closed], dtype=np.int32), sym, er
