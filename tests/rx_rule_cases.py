"""Rules, streams and helpers shared by tests/test_rx_rule_cpu.py, tests/test_rx_rule_abi.py and tests/test_gpu_rx_rule.py (numpy and
the package's host side only): the close rule of the windowed receivers as a value (include/ldpc_erasure_amd_rx_rule.h), on the
n = 200, k = 150, S = 16 of tests/rxw_cases.py."""
import numpy as np

import rxw_cases as rc

wm = rc.wm
N, K, S = rc.N, rc.K, rc.S
RANDOM_SEEDS, WRAP = rc.RANDOM_SEEDS, rc.WRAP
MAX_LATER = 1 << 30


def rules(D=1):
    """name -> rule.  The default rule spelled out; the MDS preset; close at the k-th symbol whatever follows (the block's other
    packets turn into late ones); give-up only; only c == n and the ahead limit close."""
    return {
        "default": wm.default_rule(N, K),
        "mds": wm.mds_rule(N, K, D),
        "at_k": (K, 0, K, 0),
        "giveup5": (0, 5, 0, 5),
        "never": (N, MAX_LATER, N, MAX_LATER),
    }


RULE_NAMES = tuple(rules())


# ---- the plan-edge stream of the MDS rule: events of every kind the rule adds, placed on chosen lanes of the scan's groups of 64 ----
EDGE_W, EDGE_A = rc.EDGE_W, rc.EDGE_A
EDGE_DEPTH = [(1, W) for W in EDGE_W] + [(4, 8)]   # (D, W): the plain ruled kernel, and the grouped one


def edge_stream(A):
    """(blk, sym) for mds_rule(N, K, D), D = 1 or 4, blocks 248 .. 255, 0 .. (the 8-bit wrap), in this order:
      248 with 100 symbols, 249 .. 251 with k each, 252 and 253 full.  D = 1: 249's 75th packet gives 248 up, each next block's first
          packet closes the one before at its k symbols.  D = 4: the mates 249 .. 251 do not count as later, the next group's 300th
          packet gives 248 up, and 249, 250, 251 (k symbols each) and 252 (full) close on the four packets behind it;
      254, 255, 0 full (closes by c == n across the wrap), a late packet and a bad symbol number;
      1 with 160 symbols closed by the first packet of block 1 + D; 2 completed; 3 skipped; 80 packets of 4: D = 1 gives the EMPTY
          slot 0 (block 3) up at the 75th;
      80 packets of 8 while 4 holds 80: W >= 5 gives 4 up at the 75th, and the empty 5, 6, 7 leave on the three packets behind it;
          W < 5 with A = 10 closes 4 by the ahead limit at the 11th and re-anchors at the 22nd (A = 0: late packets);
      the rest of 8 (W >= 5: a close by c == n leaves the window empty), 11 packets 50 blocks ahead (A = 10: a re-anchor of the empty
          window), the rest of that block, a full block behind it, and a short tail."""
    blk, sym = [], []

    def add(b, syms):
        syms = list(syms)
        blk.extend([b & 0xFF] * len(syms))
        sym.extend(syms)

    add(248, range(100))
    for b in (249, 250, 251):
        add(b, range(K))
    add(252, range(N))
    add(253, range(N))
    add(254, range(N))
    add(255, range(N))
    add(256, range(N))
    add(245, [1])          # late
    add(257, [0xFFFF])     # bad symbol
    add(257, range(160))
    for D in (1, 4):
        add(257 + D, [0])
    add(258, range(1, N))
    add(260, range(80))
    add(264, range(80))
    add(264, range(80, N))
    far = 314 if A > 0 else 265
    add(far, range(11))
    add(far, range(11, N))
    add(far + 1, range(N))
    add(far + 2, range(17))
    return np.array(blk, dtype=np.int64), np.array(sym, dtype=np.int64)


def edge_window(blk, sym, W, A, D, upto=None):
    """The model over the stream (its first `upto` packets) under the MDS rule."""
    w = wm.Window(N, K, W, A, D, wm.mds_rule(N, K, D))
    w.push_many(blk[:upto], sym[:upto], 1 << 30)
    return w


def cascades(w):
    """[(index of the event, length)]: a close by the give-up clause followed by `length` >= 1 closes on consecutive packets."""
    out, ev = [], w.events
    for i, why in enumerate(w.event_why):
        if why != "lo":
            continue
        j = i
        while j + 1 < len(ev) and ev[j + 1][1] == "close" and ev[j + 1][0] == ev[j][0] + 1:
            j += 1
        if j > i:
            out.append((i, j - i))
    return out


def edge_calls(blk, sym, W, A, D):
    """Call boundaries [(start, end)] that put events of the stream on lane 0, on lane 63 and on the last packet of a call, keep the
    longest cascade inside one group of 64, and end with a call of 17 packets."""
    w = edge_window(blk, sym, W, A, D)
    ev = [p for p, _ in w.events]
    P = blk.shape[0]
    cuts = {ev[9] - 64, ev[6] - 63 - 64, ev[8] + 1, P - 17}   # (events far enough apart that no cut falls between another's pair)
    cs = cascades(w)
    if cs:
        i, _ = max(cs, key=lambda t: t[1])
        cuts.add(ev[i] - 20)
    if "resync" in w.event_why:
        cuts.add(ev[w.event_why.index("resync")] - 30)
    edges = [0] + sorted(c for c in cuts if 0 < c < P) + [P]
    return list(zip(edges[:-1], edges[1:]))


def edge_facts(blk, sym, W, A, D, calls):
    """What the calls place where, from the model alone: a set of tags."""
    w = edge_window(blk, sym, W, A, D)
    ev, why, cnt0, bases = w.events, w.event_why, w.event_c, w.event_base
    facts = set()
    for (p, kind), y, c in zip(ev, why, cnt0):
        if y == "lo" and c == 0:
            facts.add("give-up close of an empty slot 0")
        if y == "lo":
            facts.add("give-up close")
        if y == "hi":
            facts.add("close at k symbols")
        if y == "resync":
            facts.add("re-anchor under c_lo == 0")
        if y == "ahead":
            facts.add("close by the ahead limit")
    if any(b > 200 for b in bases) and any(b < 50 for b in bases) and bases.index(min(bases)) > 0:
        facts.add("block numbers wrap")
    casc = {ev[i][0]: n for i, n in cascades(w)}
    for s, e in calls:
        inside = [(p - s, kind) for p, kind in ev if s <= p < e]
        for q, kind in inside:
            if q % 64 in (0, 63):
                facts.add("lane%d" % (q % 64))
            if s + q + 1 == e:
                facts.add("last packet of a call")
            n = casc.get(s + q, 0)
            if n >= 3 and q % 64 + n < 64 and s + q + n < e:
                facts.add("give-up close and three closes behind it in one group")
        if e - s < 64:
            facts.add("short call")
    return facts


def edge_facts_wanted(W, A, D):
    """The facts the stream is built to show for the object (D, W, A); see edge_stream."""
    want = {"give-up close", "close at k symbols", "block numbers wrap", "lane0", "lane63", "last packet of a call", "short call"}
    if D == 1:
        want.add("give-up close of an empty slot 0")
    if D > 1 or W >= 5:
        want.add("give-up close and three closes behind it in one group")
    if A > 0:
        want.add("re-anchor under c_lo == 0")
    if A > 0 and D == 1 and W < 5:
        want.add("close by the ahead limit")
    return want


# ---- host object and model under a rule --------------------------------------------------------------------------------------------
def host_run(pk, W, A, D=1, rule=None, max_blocks=1 << 20, cuts=(), flush=False):
    """api.FecRxWindowHost(rule=rule) over the stream, fed in the calls the cut positions make, each call repeated until it has
    consumed its piece: dict(blocks, sym, er, used (per call), stats, state, dropped); flush: the end-of-stream blocks too."""
    from ldpc_erasure_codes_amd import api
    n, S_ = N, pk.shape[1] - 8
    blocks, syms, ers, used = [], [np.zeros((0, n, S_), np.uint8)], [np.zeros((0, n), np.uint8)], []
    with api.FecRxWindowHost(n, K, S_, W, A, depth=D, rule=rule) as rx:
        edges = [0] + sorted(c for c in cuts if 0 < c < pk.shape[0]) + [pk.shape[0]]
        for a, b in zip(edges[:-1], edges[1:]):
            pos = a
            while pos < b:
                bl, sy, er, u = rx.push_many(pk[pos:b], min(max_blocks, max(1, (b - pos))))
                blocks += bl.tolist()
                syms.append(sy)
                ers.append(er)
                used.append(u)
                pos += u
        if flush:
            bl, sy, er = rx.flush()
            blocks += bl.tolist()
            syms.append(sy)
            ers.append(er)
        return dict(blocks=blocks, sym=np.concatenate(syms), er=np.concatenate(ers), used=used, stats=rx.stats(), state=rx.state(),
                    dropped=rx.dropped, rule=rx.rule)


def model_run(pk, W, A, D=1, rule=None):
    blk, sym = wm.headers(pk)
    return wm.run(blk, sym, N, K, W, A, D=D, rule=rule)


# ---- the quality claim: Reed-Solomon shaped blocks on the burst channel --------------------------------------------------------------
RS_N, RS_K = 255, 192
QUALITY_SEEDS, QUALITY_DW, QUALITY_BLOCKS, QUALITY_A = (79, 81), ((1, 16), (8, 16)), 256, 10


def rs_wire(nblocks, D, n=RS_N, block0=0):
    """(blk, sym) of nblocks blocks on the in-order depth-D wire: one packet of every block of a group in turn."""
    assert nblocks % D == 0
    g, i, j = np.meshgrid(np.arange(nblocks // D), np.arange(n), np.arange(D), indexing="ij")
    return ((block0 + g * D + j).ravel() & 0xFF).astype(np.int64), i.ravel().astype(np.int64), (g * D + j).ravel()


def burst_keep(seed, P):
    """The Gilbert-Elliott trace of the README's RS row by wire position: True = the packet arrives."""
    from ldpc_erasure_codes_amd import synth
    return np.asarray(synth.erasures_bursty(seed, 0, P, 1, 0.13, 0.8, 10.0)).reshape(-1)[:P] == 0


def quality_stream(seed, D, nblocks=QUALITY_BLOCKS):
    """The received (blk, sym) and, per sent block, how many of its packets arrived."""
    blk, sym, serial = rs_wire(nblocks, D)
    keep = burst_keep(seed, blk.shape[0])
    return blk[keep], sym[keep], np.bincount(serial[keep], minlength=nblocks)


def delivered(closed, k=RS_K):
    """Blocks handed out with k or more distinct symbols."""
    return sum(1 for _, win in closed if len(win) >= k)
