"""Test streams for the multi-flow receiver (include/ldpc_erasure_amd_flows.h), built on the host alone: numpy, the CPU oracle's
encoder, api.fec_packetize and a numpy channel.  The reference side of the tests -- one host api.FecRx per flow, fed with the same
call boundaries the device object gets -- lives here too, so that what a stream exercises (staging rows, calls that close nothing,
flows that stop at max_blocks_per_flow, block numbers that wrap) can be asserted without a GPU (tests/test_flow_streams_cpu.py).

Nothing in this module touches the code under test (csrc/wire_dev.hip's flows entry points)."""
import numpy as np

from ldpc_erasure_codes_amd import api


def min_parity_rx(n, k):
    """k + round(0.2 (n - k)): a block that stays at or below this many received packets never closes (the draft's rule stalls)."""
    return k + int(np.floor((n - k) * 0.2 + 0.5))


def encode_packets(oc, code, S, F, seed, block0=0):
    """F random frames through the oracle's encoder and the host packetiser: uint8 [F * n][8 + S] in transmission order."""
    rng = np.random.default_rng(seed)
    frames = np.zeros((F, code.n, S), dtype=np.uint8)
    for f in range(F):
        src = rng.integers(0, 256, size=(code.k, S), dtype=np.uint8)
        frames[f] = oc.encode(src[:, 0]).reshape(code.n, 1) if S == 1 else oc.encode(src)
    if F == 0:
        return np.zeros((0, 8 + S), dtype=np.uint8)
    return api.fec_packetize(frames, 1, block0)


def channel(pk, n, seed, loss=(0.0, 0.05, 0.1, 0.15), window=120, dup=0.02, dup_flip=True, bad_sym=0.005, foreign=0.005):
    """A lossy, re-ordering, duplicating channel.  Per frame a loss rate from `loss`; every packet moves up to `window` places; a
    fraction `dup` of the kept packets is sent again a little later (with a flipped payload if dup_flip: the receiver keeps the last
    copy); a fraction gets a symbol number >= n, another a random block number.  Returns (packets, received): received[f] = distinct
    symbols of frame f that arrive with their header intact.  The random draws do not depend on the payload length."""
    rng = np.random.default_rng(seed)
    P = pk.shape[0]
    F = P // n
    if P == 0:
        return pk.copy(), np.zeros(0, dtype=np.int64)
    frame = np.arange(P) // n
    rate = np.asarray(loss, dtype=np.float64)[rng.integers(0, len(loss), size=F)][frame]
    keep = rng.random(P) >= rate
    kept, origin = pk[keep], np.flatnonzero(keep)
    K = kept.shape[0]
    di = rng.integers(0, K, size=max(1, int(K * dup))) if dup > 0 else np.zeros(0, dtype=np.int64)
    d = kept[di].copy()
    if dup_flip:
        d[:, 8:] ^= 0x5A
    pos = np.concatenate([np.arange(K, dtype=np.float64), di + rng.integers(1, 64, size=di.shape[0]).astype(np.float64)])
    pos = pos + rng.random(pos.shape[0]) * window
    order = np.argsort(pos, kind="stable")
    out = np.ascontiguousarray(np.concatenate([kept, d])[order])
    origin = np.concatenate([origin, origin[di]])[order]
    bad = rng.random(out.shape[0]) < bad_sym
    out[bad, 1] = 0xFF                                    # symbol number >= 0xff00 >= n
    fgn = rng.random(out.shape[0]) < foreign
    out[fgn, 2] = rng.integers(0, 256, size=int(fgn.sum()), dtype=np.uint8)
    good = origin[~bad & ~fgn]
    received = np.array([np.unique(good[good // n == f]).size for f in range(F)], dtype=np.int64)
    return out, received


def flow_begin_of(segments):
    """The packet array of one call and its flow_begin: the flows' segments laid side by side."""
    lens = [s.shape[0] for s in segments]
    return np.ascontiguousarray(np.concatenate(segments)), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def reference_calls(flows, n, k, S, seed, sizes, max_blocks):
    """Every flow's stream through a host api.FecRx of its own, in calls of mixed per-flow segment sizes.  Per call: mb, and per flow
    pos (where its segment starts in its stream), c (packets offered), used, blocks, sym, er, dropped.  Then every flow's flushes."""
    rng = np.random.default_rng(seed)
    nf = len(flows)
    rxs = [api.FecRx(n, k, S) for _ in range(nf)]
    pos = [0] * nf
    calls = []
    while any(pos[f] < flows[f].shape[0] for f in range(nf)):
        mb = int(rng.choice(max_blocks))
        per = []
        for f in range(nf):
            c = min(int(rng.choice(sizes)), flows[f].shape[0] - pos[f])
            if c > 0:
                b, sym, er, used = rxs[f].push_many(flows[f][pos[f]:pos[f] + c], mb)
                assert used > 0
            else:
                b, sym, er, used = np.zeros(0, np.int32), np.zeros((0, n, S), np.uint8), np.zeros((0, n), np.uint8), 0
            per.append(dict(pos=pos[f], c=c, used=used, blocks=b.copy(), sym=sym, er=er, dropped=rxs[f].dropped))
            pos[f] += used
        calls.append(dict(mb=mb, flows=per))
    flushes = []
    for f in range(nf):
        fl = []
        while True:
            r = rxs[f].flush()
            if r is None:
                break
            fl.append(r)
        flushes.append(fl)
        rxs[f].close()
    return calls, flushes


def call_packets(flows, call):
    """(packets, flow_begin) of one call of reference_calls."""
    return flow_begin_of([flows[f][c["pos"]:c["pos"] + c["c"]] for f, c in enumerate(call["flows"])])


def expected(call, n, S):
    """What the flows object must return for the call: closes [nflows], blocks [T], sym [T][n][S], er [T][n], consumed, dropped."""
    per = call["flows"]
    return dict(closes=np.array([len(c["blocks"]) for c in per], dtype=np.int32),
                blocks=np.concatenate([c["blocks"] for c in per]).astype(np.int32),
                sym=np.concatenate([c["sym"] for c in per]).reshape(-1, n, S), er=np.concatenate([c["er"] for c in per]).reshape(-1, n),
                consumed=np.array([c["used"] for c in per], dtype=np.int64), dropped=np.array([c["dropped"] for c in per], dtype=np.int64))


def carried_blocks(pk, calls, f, n):
    """Closed blocks of flow f that hold more received symbols than the packets of their own call brought: the rest was received by
    an earlier call and waited in a staging plane."""
    sym = pk[:, 0].astype(np.int64) | (pk[:, 1].astype(np.int64) << 8)
    blk = pk[:, 2].astype(np.int64)
    count = 0
    for call in calls:
        c = call["flows"][f]
        s, b = sym[c["pos"]:c["pos"] + c["used"]], blk[c["pos"]:c["pos"] + c["used"]]
        for j, bn in enumerate(c["blocks"]):
            here = np.unique(s[(b == bn) & (s < n)]).size
            count += int(n - int(c["er"][j].sum()) > here)
    return count


# ---- the streams of tests/test_gpu_flows.py -----------------------------------------------------------------------------------
# mixed: the random (300,200) code; a flow that is always empty, a single block, a few, a run that wraps the block number, a long one
MIXED = dict(F=(0, 1, 7, 20, 40), block0=(0, 0, 0, 250, 0), sizes=(0, 1, 17, 300, 1111, 4000), max_blocks=(1, 2, 3, 64))


def mixed_flows(oc, code, S, seed=1000):
    """[(packets, received)] of the MIXED flows, each with its own channel seed."""
    return [channel(encode_packets(oc, code, S, F, seed + 10 * f, b0), code.n, seed + 10 * f + 1)
            for f, (F, b0) in enumerate(zip(MIXED["F"], MIXED["block0"]))]


# (the 20 % flow's seed is one at which every block keeps more than k + 0.2 (n - k) = 1632 packets: at that rate half of all blocks do not)
# builtin: 3 flows x 6 frames of the (2040,1530) code; the last flow at 20 % loss (with max_sweeps = 1 it reaches tier 2 and the ML stage)
BUILTIN = dict(F=6, loss=((0.0, 0.05, 0.1), (0.1, 0.15), (0.2,)), seeds=(2001, 2011, 4481), sizes=(3000, 9000, 30000), max_blocks=(3, 64))


def builtin_flows(oc, code, S):
    return [channel(encode_packets(oc, code, S, BUILTIN["F"], sd, 0), code.n, sd + 1, loss=ls, bad_sym=0.001, foreign=0.001)
            for ls, sd in zip(BUILTIN["loss"], BUILTIN["seeds"])]


def equal_flows(oc, code, S, nflows, F, seed, **chan):
    """nflows flows of F frames each, flow f numbered from block f on."""
    return [channel(encode_packets(oc, code, S, F, seed + 10 * f, f & 0xFF), code.n, seed + 10 * f + 1, **chan) for f in range(nflows)]


# many: more flows than a wavefront has lanes, everything in one call
MANY = dict(nflows=130, F=3, sizes=(4000,), max_blocks=(64,))
# words: word-sized symbols (S = 20 with symbol unit 4)
WORDS = dict(nflows=3, F=5, sizes=(17, 300, 1111), max_blocks=(1, 2, 64))
# heavy: the MIXED layout for test_gpu_sender.heavy_code() (48,24), whose blocks close only with 44 of their 48 packets
HEAVY = dict(loss=(0.0, 0.02), window=6, dup=0.02, bad_sym=0.0, foreign=0.0)

_SCENARIOS = {}


def scenario(name, oc, code, S):
    """(The seeds of the call boundaries are ones at which tests/test_flow_streams_cpu.py's conditions hold.)
    dict(flows=[packets per flow], received=[per flow, per frame], F=[frames per flow], calls, flushes) of a named stream set;
    built once per process.  The channel's and the call boundaries' random draws do not depend on S."""
    key = (name, code.n, code.k, S)
    if key in _SCENARIOS:
        return _SCENARIOS[key]
    if name == "mixed":
        fl, F, sizes, mbs, seed = mixed_flows(oc, code, S), MIXED["F"], MIXED["sizes"], MIXED["max_blocks"], 8
    elif name == "heavy":
        fl = [channel(encode_packets(oc, code, S, F, 5000 + 10 * f, b0), code.n, 5001 + 10 * f, **HEAVY)
              for f, (F, b0) in enumerate(zip(MIXED["F"], MIXED["block0"]))]
        F, sizes, mbs, seed = MIXED["F"], MIXED["sizes"], MIXED["max_blocks"], 12
    elif name == "builtin":
        fl, F, sizes, mbs, seed = builtin_flows(oc, code, S), (BUILTIN["F"],) * 3, BUILTIN["sizes"], BUILTIN["max_blocks"], 9
    elif name == "many":
        fl = equal_flows(oc, code, S, MANY["nflows"], MANY["F"], 3000)
        F, sizes, mbs, seed = (MANY["F"],) * MANY["nflows"], MANY["sizes"], MANY["max_blocks"], 10
    elif name == "words":
        fl = equal_flows(oc, code, S, WORDS["nflows"], WORDS["F"], 4000)
        F, sizes, mbs, seed = (WORDS["F"],) * WORDS["nflows"], WORDS["sizes"], WORDS["max_blocks"], 11
    else:
        raise KeyError(name)
    flows = [f[0] for f in fl]
    calls, flushes = reference_calls(flows, code.n, code.k, S, seed, sizes, mbs)
    sc = dict(flows=flows, received=[f[1] for f in fl], F=tuple(F), calls=calls, flushes=flushes)
    _SCENARIOS[key] = sc
    return sc


def closed_per_flow(sc):
    return [sum(len(c["flows"][f]["blocks"]) for c in sc["calls"]) + len(sc["flushes"][f]) for f in range(len(sc["flows"]))]
