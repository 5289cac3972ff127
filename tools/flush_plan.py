"""Host model of the multi-flow receiver's batch flush (include/ldpc_erasure_amd_flows_flush.h) and the stream sets of its tests,
built on the host alone.

The model is the mirror rule of csrc/wire.cpp's ldpc_amd_fec_rx_flush replayed per flow: a flow is (cur_block, cur_cnt, next_cnt) --
what FecRxFlows.pending() returns, and all the rule looks at -- its next block is cur_block + 1 modulo 256.  plan() gives the slot
order, closes and the state after a flush_many call.  tests/test_flush_plan_cpu.py checks it against api.FecRx drained per flow; the
GPU tests take slot order from it.

Nothing in this module touches the code under test (csrc/wire_dev.hip's flush entry points)."""
import numpy as np

from ldpc_erasure_codes_amd import api

import flow_streams as fs


def open_blocks(cur, cc, nc):
    """How many flushes of a flow in this state return a block: 0, 1 or 2."""
    if cur < 0 or (cc == 0 and nc == 0):
        return 0
    return 2 if nc > 0 else 1


def plan(state, flows=None, rounds=2):
    """state: (cur_block [nflows], cur_cnt [nflows], next_cnt [nflows]); flows: the list of the call (None: all flows).
    Returns dict(slots=[(flow, block)] in slot order, closes int32 [nsel], state=the three arrays after the call)."""
    cur, cc, nc = (np.array(a, dtype=np.int32).copy() for a in state)
    sel = range(len(cur)) if flows is None else [int(f) for f in flows]
    assert rounds in (1, 2) and len(set(sel)) == len(sel) and all(0 <= f < len(cur) for f in sel)
    slots, closes = [], []
    for f in sel:
        c = 0
        while c < rounds and cur[f] >= 0 and (cc[f] != 0 or nc[f] != 0):
            slots.append((f, int(cur[f])))
            cur[f], cc[f], nc[f] = (cur[f] + 1) & 0xFF, nc[f], 0      # wire.cpp: close_current
            c += 1
        closes.append(c)
    return dict(slots=slots, closes=np.array(closes, dtype=np.int32), state=(cur, cc, nc))


def state_of(rxs_flushes):
    """The model's state of host receivers from what draining them returned: per flow the list [(block, sym, er)] of its flushes.
    (The counts are only known as zero / non-zero: the received symbols of the block, which is all the rule asks.)"""
    nf = len(rxs_flushes)
    cur, cc, nc = np.full(nf, -1, np.int32), np.zeros(nf, np.int32), np.zeros(nf, np.int32)
    for f, fl in enumerate(rxs_flushes):
        assert len(fl) <= 2
        if fl:
            cur[f] = fl[0][0]
            cc[f] = int((fl[0][2] == 0).sum())
        if len(fl) == 2:
            assert fl[1][0] == (fl[0][0] + 1) & 0xFF
            nc[f] = int((fl[1][2] == 0).sum())
            assert nc[f] > 0
    return cur, cc, nc


# ---- the stream sets of tests/test_gpu_flows_flush.py ---------------------------------------------------------------------------
def tail_flow(oc, code, S, seed, block0, keep):
    """One flow of len(keep) consecutive blocks sent in order without reordering or duplicates; of block j arrive all n packets
    (keep[j] None), only the first keep[j] (an int), or each with probability 1 - keep[j] (a float: a loss rate).  A block that got
    all n packets closes on the way, no other one does: what is left open is known."""
    pk = fs.encode_packets(oc, code, S, len(keep), seed, block0)
    n = code.n
    rng = np.random.default_rng(seed + 1)
    parts = []
    for j, kp in enumerate(keep):
        blk = pk[j * n:(j + 1) * n]
        parts.append(blk if kp is None else (blk[rng.random(n) >= kp] if isinstance(kp, float) else blk[:kp]))
    return np.ascontiguousarray(np.concatenate(parts))


def kinds(flushes, k):
    """Which of the four flow kinds of the issue a set of per-flow flushes holds: flows with two open blocks, with an empty current
    and a non-empty next block, with nothing open, and blocks with fewer than k received symbols."""
    two = [f for f, fl in enumerate(flushes) if len(fl) == 2 and not fl[0][2].all()]
    empty_cur = [f for f, fl in enumerate(flushes) if len(fl) == 2 and fl[0][2].all() and not fl[1][2].all()]
    nothing = [f for f, fl in enumerate(flushes) if len(fl) == 0]
    short = [(f, j) for f, fl in enumerate(flushes) for j, (_, _, er) in enumerate(fl) if int((er == 0).sum()) < k]
    return dict(two=two, empty_cur=empty_cur, nothing=nothing, short=short)


_SCENARIOS = {}


def scenario(name, oc, code, S):
    """flow_streams.scenario's dict for the stream sets of the flush tests; built once per process.
    mixed:   flow_streams' MIXED flows, then four flows whose tails are known: a complete block, a wholly lost one and 30 packets of
             the one after it (empty current block, non-empty next one); 150 < k packets of one block (undecodable); two complete
             blocks across the wrap of the block number and all but 20 packets of the next (one open block); a complete block, 90 %
             of the next and 40 packets of the one after it (two open blocks, both with packets).
    builtin: 4 flows of the (2040,1530) code with the tails of the issue: complete, tier 2, ML stage, undecodable.
    many / crowd: 130 / 300 flows, every flow left with one or two open blocks (or none)."""
    key = (name, code.n, code.k, S)
    if key in _SCENARIOS:
        return _SCENARIOS[key]
    n, k = code.n, code.k
    if name == "mixed":
        flows = [f[0] for f in fs.mixed_flows(oc, code, S)]
        flows += [tail_flow(oc, code, S, 7000, 3, (None, 0, 30)), tail_flow(oc, code, S, 7010, 0, (150,)),
                  tail_flow(oc, code, S, 7020, 254, (None, None, n - 20)), tail_flow(oc, code, S, 7030, 100, (None, 0.1, 40))]
        sizes, mbs, seed = fs.MIXED["sizes"], fs.MIXED["max_blocks"], 8
    elif name == "builtin":
        # a block complete but for its last packet (one with all n closes by itself); 23 % lost: more erasures than a block that
        # closes on the way can have (n - k - 0.2 (n - k) = 408), so more than tier 1 of the S = 1024 plan takes; 20 % lost: one sweep
        # leaves the frame to the ML stage; fewer than k packets, and 25 of the block after it: undecodable
        flows = [tail_flow(oc, code, S, 7100, 0, (None, n - 1)), tail_flow(oc, code, S, 7110, 9, (0.23,)),
                 tail_flow(oc, code, S, 7120, 200, (None, 0.20)), tail_flow(oc, code, S, 7130, 255, (k - 40, 25))]
        sizes, mbs, seed = (3000, 9000), (3, 64), 9
    elif name in ("many", "crowd"):
        nf = 130 if name == "many" else 300
        rng = np.random.default_rng(77 if name == "many" else 78)
        # 2 frames per flow through the lossy channel, cut at a random point of the second frame (or before the first packet)
        fl = fs.equal_flows(oc, code, S, nf, 2, 7200 if name == "many" else 7300)
        flows = [f[0][:int(rng.choice((0, 40, n // 2, n + 20, n + n // 2, f[0].shape[0])))] for f in fl]
        sizes, mbs, seed = (4000,), (64,), 10
    else:
        raise KeyError(name)
    calls, flushes = fs.reference_calls(flows, n, k, S, seed, sizes, mbs)
    sc = dict(flows=flows, calls=calls, flushes=flushes)
    _SCENARIOS[key] = sc
    return sc


def host_receivers(sc, n, k, S):
    """One api.FecRx per flow, fed the stream set's calls: the receivers in the state in which the flush tests drain the device."""
    rxs = [api.FecRx(n, k, S) for _ in sc["flows"]]
    for call in sc["calls"]:
        for f, c in enumerate(call["flows"]):
            if c["c"] > 0:
                rxs[f].push_many(sc["flows"][f][c["pos"]:c["pos"] + c["c"]], call["mb"])
    return rxs


def drain(rx, rounds=2):
    """[(block, sym, er)] of up to `rounds` flushes of one host receiver."""
    fl = []
    for _ in range(rounds):
        r = rx.flush()
        if r is None:
            break
        fl.append(r)
    return fl
