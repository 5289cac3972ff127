"""What the two multi-flow device receivers answer, as a table (tests/test_gpu_rx_flows_refusals.py compares the build under test with
tests/rx_flows_refusals_pinned.json, recorded from the build before their host code was folded into one call skeleton,
csrc/rx_flows_host.h):

    plain  ldpc_amd_fec_rx_flows_...    two open blocks per flow      win  ldpc_amd_fec_rxw_flows_...    a window of W open blocks per flow

each through its eight entry points: push_many, decode_many, push_mixed, decode_mixed, flush_many, decode_flush_many, create, destroy.

run(ctx, ctx4) first sends every case of CASES through the raw ctypes entry point: one row [name, status, text of
ldpc_amd_last_error, what the case did to the object, status and outputs of a good call behind it].  What the case did: the object's
whole visible state -- pending, dropped / stats / state per flow, unrouted -- and the words of the four ..._info calls are read in
front of the case and behind it; the row says "unchanged", or holds the text read behind it.  The good call goes through the same
entry point; its outputs are recorded as a digest, and behind it a digest of the state and info text (the text itself stands in the
GOOD rows): the object is still usable and answers, and stands, as before.  Then GOOD: sequences of good calls on fresh objects -- a
call that closes nothing, a call that stops at max_blocks_per_flow, a batch flush of one flow and of all -- segmented and mixed (with
a packet of no flow and with `left`), at S = 16 and at S = 20 under symbol unit 4, from packets 4 but not 8 bytes aligned, with the
packets-in decoder switched off, and for the windowed object at depth 1 and 2 under the default rule and the MDS preset; each call a
row [name, status, outputs as a digest, state and info text].  ctx4: a context at symbol unit 4.

No case reaches a launch with a bad pointer: every bad pointer is null or host memory, which the library refuses first.

    python tests/rx_flows_refusal_cases.py --lib PATH/libldpc_erasure_amd.so --out FILE     records the table of that build"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from ldpc_erasure_codes_amd import api  # noqa: E402
from code_helpers import random_code  # noqa: E402

KINDS = ("plain", "win")
PRE = {"plain": "ldpc_amd_fec_rx_flows_", "win": "ldpc_amd_fec_rxw_flows_"}
PACKET_CALLS = ("push_many", "decode_many", "push_mixed", "decode_mixed")
DECODE_CALLS = ("decode_many", "decode_mixed", "decode_flush_many")
MIXED_CALLS = ("push_mixed", "decode_mixed")
FLUSH_CALLS = ("flush_many", "decode_flush_many")
NF, N, K, W, AHEAD, MB = 3, 40, 24, 4, 10, 2   # flows (flow 1 gets no packet), the code, the window, max_blocks_per_flow
BIG = 1 << 31


def _cases():
    """(name, kind, entry point, arguments that differ from the good call).  Pointers: "dev" (default), "host", None, or
    ("dev", byte offset)."""
    out = []

    def add(name, calls, kinds=KINDS, **kw):
        for kind in kinds:
            for call in calls:
                out.append((f"{kind} {call}: {name}", kind, call, dict(kw)))

    seg, mixed, push, dec = ("push_many", "decode_many"), MIXED_CALLS, ("push_many", "push_mixed"), ("decode_many", "decode_mixed")
    # ---- the packet calls: single faults
    add("null flow_begin", seg, fb=None)
    add("flow_begin[0] != 0", seg, fb=[1, 1, 1, 1])
    add("decreasing flow_begin", seg, fb=[0, 5, 4, 6])
    add("2^31 packets, null pointers", PACKET_CALLS, P=BIG, packets=None, sym=None, er=None, out=None, flow_of=None)
    add("max_blocks_per_flow = 0", PACKET_CALLS, mb=0)
    add("nflows * max_blocks * n too large", PACKET_CALLS, mb=BIG // (NF * N) + 1)
    add("no packets, null pointers", PACKET_CALLS, P=0, packets=None, sym=None, er=None, out=None, flow_of=None)
    add("no packets", PACKET_CALLS, P=0)
    add("null packets", PACKET_CALLS, packets=None)
    add("host packets", PACKET_CALLS, packets="host")
    add("null sym_batch", push, sym=None)
    add("host sym_batch", push, sym="host")
    add("host erased_batch", push, er="host")
    add("null out", dec, out=None)
    add("host out", dec, out="host")
    add("host result array", dec, status="host")
    add("null flow_of", mixed, flow_of=None)
    add("host flow_of", mixed, flow_of="host")
    add("misaligned flow_of", mixed, flow_of=("dev", 2))
    add("host left", mixed, left="host")
    add("unknown code handle", DECODE_CALLS, code=999)
    add("a code of another (n, k)", DECODE_CALLS, code="other")
    add("max_sweeps = 0", DECODE_CALLS, max_sweeps=0)
    add("S = 20 at symbol unit 16", DECODE_CALLS, obj="s20")
    # ---- the packet calls: two faults in one call, one pair per adjacent pair of checks
    add("unknown code handle + decreasing flow_begin", ("decode_many",), code=999, fb=[0, 5, 4, 6])
    add("unknown code handle + 2^31 packets", ("decode_mixed",), code=999, P=BIG)
    add("decreasing flow_begin + max_blocks_per_flow = 0", seg, fb=[0, 5, 4, 6], mb=0)
    add("2^31 packets + max_blocks_per_flow = 0", PACKET_CALLS, P=BIG, mb=0)
    add("nflows * max_blocks * n too large + null sym_batch", push, mb=BIG // (NF * N) + 1, sym=None)
    add("max_blocks_per_flow = 0 + no packets", PACKET_CALLS, mb=0, P=0)
    add("no packets + unknown code handle", dec, P=0, code=999)
    add("no packets + a code of another (n, k)", dec, P=0, code="other")
    add("no packets + host out", dec, P=0, out="host")
    add("no packets + host sym_batch", push, P=0, sym="host")
    add("null sym_batch + host packets", push, sym=None, packets="host")
    add("host packets + misaligned flow_of", mixed, packets="host", flow_of=("dev", 2))
    add("host flow_of + host left", mixed, flow_of="host", left="host")
    add("misaligned flow_of + host left", mixed, flow_of=("dev", 2), left="host")
    add("a code of another (n, k) + max_sweeps = 0", dec, code="other", max_sweeps=0)
    add("S = 20 at symbol unit 16 + max_sweeps = 0", dec, obj="s20", max_sweeps=0)
    add("max_sweeps = 0 + host out", dec, max_sweeps=0, out="host")
    add("host out + host packets", dec, out="host", packets="host")
    # ---- the batch flush
    add("nsel = -1", FLUSH_CALLS, flows=[0], nsel=-1)
    add("nsel > nflows", FLUSH_CALLS, flows=[0, 1, 2, 0], nsel=4)
    add("flow -1", FLUSH_CALLS, flows=[0, -1])
    add("flow nflows", FLUSH_CALLS, flows=[NF])
    add("a flow twice", FLUSH_CALLS, flows=[2, 0, 2])
    add("rounds = 0", FLUSH_CALLS, ("plain",), rounds=0)
    add("rounds = 3", FLUSH_CALLS, ("plain",), rounds=3)
    add("an empty object", FLUSH_CALLS, obj="empty")
    add("null sym_batch", ("flush_many",), sym=None)
    add("host erased_batch", ("flush_many",), er="host")
    add("host out", ("decode_flush_many",), out="host")
    add("rounds = 0 + a flow twice", FLUSH_CALLS, ("plain",), rounds=0, flows=[0, 0])
    add("nsel > nflows + flow nflows", FLUSH_CALLS, flows=[NF, 0, 1, 2], nsel=4)
    add("flow -1 + a flow twice", FLUSH_CALLS, flows=[-1, 0, 0])
    add("a flow twice + flow -1", FLUSH_CALLS, flows=[0, 0, -1])
    add("a flow twice + null sym_batch", ("flush_many",), flows=[0, 0], sym=None)
    add("null sym_batch + host erased_batch", ("flush_many",), sym=None, er="host")
    add("host sym_batch + an empty object", ("flush_many",), obj="empty", sym="host")
    add("a flow twice + unknown code handle", ("decode_flush_many",), flows=[0, 0], code=999)
    add("unknown code handle + max_sweeps = 0", ("decode_flush_many",), code=999, max_sweeps=0)
    add("an empty object + host out", ("decode_flush_many",), obj="empty", out="host")
    # ---- create and destroy
    add("nflows = 0", ("create",), nflows=0)
    add("nflows = 4097", ("create",), nflows=4097)
    add("k = n", ("create",), k=N)
    add("S = 0", ("create",), S=0)
    add("null out", ("create",), null_out=True)
    add("null out + nflows = 0", ("create",), null_out=True, nflows=0)
    add("window = 1", ("create",), ("win",), window=1)
    add("window = 33", ("create",), ("win",), window=33)
    add("ahead_limit = -1", ("create",), ("win",), ahead=-1)
    add("depth 3", ("create",), ("win",), depth=3)
    add("2 * depth > window", ("create",), ("win",), depth=4)
    add("an invalid rule", ("create",), ("win",), rule=(N + 1, 1, 0, 1))
    add("nflows = 0 + window = 1", ("create",), ("win",), nflows=0, window=1)
    add("window = 1 + depth 3", ("create",), ("win",), window=1, depth=3)
    add("depth 3 + an invalid rule", ("create",), ("win",), depth=3, rule=(N + 1, 1, 0, 1))
    add("null object", ("destroy",))
    return out


CASES = _cases()


def _sha(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


class _Env:
    """One context's codes, packets and arrays."""

    def __init__(self, ctx, torch, S):
        self.ctx, self.L, self.torch, self.S = ctx, api.load_library(), torch, S
        self.dev = torch.device("cuda", ctx.device)
        self.code = ctx.register_code(random_code(n=N, k=K, seed=5))
        self.other = ctx.register_code(random_code(n=N - 4, k=K, seed=6))
        # flow 0: blocks 0 .. 5, flow 2: blocks 250 .. 255, 0, 1 (the wrap); one packet in 25 lost; flow 1: nothing
        rng = np.random.default_rng(17)
        g = torch.Generator(device=self.dev).manual_seed(23)
        self.streams = {}
        for f, (F, b0) in ((0, (6, 0)), (2, (8, 250))):
            src = torch.randint(0, 256, (F, K, S), dtype=torch.uint8, device=self.dev, generator=g)
            pk = ctx.fec_encode_packets_device(self.code, src, 1, b0)
            keep = np.flatnonzero(rng.random(F * N) >= 0.04)
            self.streams[f] = pk[torch.from_numpy(keep).to(self.dev)].contiguous()
        ctx.synchronize()
        self.bytes = 1 << 16
        self.bufs = {k: torch.zeros(self.bytes, dtype=torch.uint8, device=self.dev) for k in ("packets", "flow_of", "sym", "er", "out", "left", "eo")}
        self.i32 = {k: torch.zeros(64, dtype=torch.int32, device=self.dev) for k in ("sweeps", "residual", "status", "rsrc")}
        self.host = np.zeros(self.bytes, dtype=np.uint8)

    def batch(self, lo, hi, mixed, misalign=0):
        """Packets lo[f] .. hi[f] - 1 of every flow's stream, segmented (-> flow_begin) or interleaved (-> flow_of, with two
        packets of no flow), written into the packet buffer `misalign` bytes in.  Returns (P, flow_begin, flow_of)."""
        torch = self.torch
        parts = {f: self.streams[f][lo[f]:hi[f]] for f in (0, 2)}
        fb = np.array([0, len(parts[0]), len(parts[0]), len(parts[0]) + len(parts[2])], dtype=np.int64)
        pk = torch.cat([parts[0], parts[2]])
        fo = np.repeat(np.array([0, 2], dtype=np.int32), [len(parts[0]), len(parts[2])])
        if mixed:   # a shuffled sequence of the flow numbers; the i-th packet with number f is the flow's i-th: arrival order inside a flow
            lab = np.random.default_rng(3).permutation(fo)
            nth = np.zeros(len(lab), dtype=np.int64)
            for f in (0, 2):
                nth[lab == f] = np.arange(int((lab == f).sum())) + (0 if f == 0 else len(parts[0]))
            pk, fo = pk[torch.from_numpy(nth).to(self.dev)], lab.copy()
            if len(fo) > 4:   # two packets of no flow: a negative number and one past the last flow
                fo[1], fo[len(fo) // 2] = -1, NF + 4
        P = int(pk.shape[0])
        flat = pk.reshape(-1)
        self.bufs["packets"][misalign:misalign + flat.numel()] = flat
        self.bufs["flow_of"][:4 * P] = torch.from_numpy(fo).to(self.dev).view(torch.uint8)
        return P, fb, fo

    def ptr(self, what, p):
        if p is None:
            return None
        where, off = p if isinstance(p, tuple) else (p, 0)
        if where == "host":
            return self.host.ctypes.data + off
        t = self.i32[what] if what in self.i32 else self.bufs[what]
        return t.data_ptr() + off

    def create(self, kind, nflows=NF, n=N, k=K, S=None, window=W, ahead=AHEAD, depth=1, rule=None, null_out=False):
        h = C.c_void_p()
        out = None if null_out else C.byref(h)
        S = self.S if S is None else S
        if kind == "plain":
            rc = self.L.ldpc_amd_fec_rx_flows_create(self.ctx._h, nflows, n, k, S, out)
        elif rule is not None:
            rc = self.L.ldpc_amd_fec_rxw_flows_create_rule(self.ctx._h, nflows, n, k, S, window, ahead, depth, C.byref(api.RxRule(*rule)), out)
        elif depth != 1:
            rc = self.L.ldpc_amd_fec_rxw_flows_create_depth(self.ctx._h, nflows, n, k, S, window, ahead, depth, out)
        else:
            rc = self.L.ldpc_amd_fec_rxw_flows_create(self.ctx._h, nflows, n, k, S, window, ahead, out)
        return rc, h

    def destroy(self, kind, h):
        getattr(self.L, PRE[kind] + "destroy")(h)

    def call(self, kind, h, call, P, fb, packets="dev", flow_of="dev", sym="dev", er="dev", out="dev", status="dev", left=None, mb=MB, code=None,
             max_sweeps=10, flows=None, nsel=None, rounds=2, window=W):
        """One raw call.  Returns (status, host outputs).  P: the mixed call's packet count; a segmented call's is its flow_begin's."""
        fn = getattr(self.L, PRE[kind] + call)
        code = {None: self.code, "other": self.other}.get(code, code)
        slots = max(NF * max(window, 2), 1)
        o = {"blocks": np.full(slots, -7, dtype=np.int32), "closes": np.full(NF + 1, -7, dtype=np.int32), "consumed": np.full(NF, -7, dtype=np.int64),
             "offered": np.full(NF, -7, dtype=np.int64)}
        hp = {k: v.ctypes.data for k, v in o.items()}
        res = (self.ptr("out", out), self.ptr("sweeps", "dev"), self.ptr("residual", "dev"), self.ptr("status", status), self.ptr("eo", "dev"),
               self.ptr("rsrc", "dev"))
        if call in FLUSH_CALLS:
            sel = None if flows is None else np.ascontiguousarray(flows, dtype=np.int32)
            ns = (NF if sel is None else len(sel)) if nsel is None else nsel
            a = [h] + ([code] if call == "decode_flush_many" else []) + [None if sel is None else sel.ctypes.data, ns] + ([rounds] if kind == "plain" else [])
            a += [max_sweeps, 1, *res] if call == "decode_flush_many" else [self.ptr("sym", sym), self.ptr("er", er)]
            return fn(*a, hp["blocks"], hp["closes"]), o
        fbk = None if fb is None else np.ascontiguousarray(fb, dtype=np.int64)
        where = [self.ptr("flow_of", flow_of), P] if call in MIXED_CALLS else [None if fbk is None else fbk.ctypes.data]
        a = [h] + ([code] if call in DECODE_CALLS else []) + [self.ptr("packets", packets)] + where
        a += [max_sweeps, 1, *res] if call in DECODE_CALLS else [self.ptr("sym", sym), self.ptr("er", er)]
        a += [hp["blocks"], hp["closes"], mb, hp["consumed"]]
        if call in MIXED_CALLS:
            a += [hp["offered"], self.ptr("left", left)]
        return fn(*a), o

    def digest(self, call, T, o, P, left, nsel=NF, short=False):
        """The outputs of a good call that returned T, as text."""
        self.ctx.synchronize()
        n, S = N, self.S
        parts = [o["blocks"][:T]]
        if call in DECODE_CALLS:
            st = self.i32["status"][:T].cpu().numpy()
            frames = self.bufs["out"][:T * n * S].cpu().numpy().reshape(T, n * S)
            parts += [st, self.i32["sweeps"][:T].cpu().numpy(), self.bufs["eo"][:T * n].cpu().numpy(), frames[st == 0]]
        else:
            parts += [self.bufs["sym"][:T * n * S].cpu().numpy(), self.bufs["er"][:T * n].cpu().numpy()]
        host = [o["closes"][:nsel]] + ([o["consumed"]] if call in PACKET_CALLS else []) + ([o["offered"]] if call in MIXED_CALLS else [])
        if call in MIXED_CALLS and left:
            parts.append(self.bufs["left"][:P].cpu().numpy())
        if short:   # every output in the digest
            return f"T={T} sha={_sha(*host, *parts)}"
        text = f"T={T} closes={host[0].tolist()}" + (f" consumed={host[1].tolist()}" if call in PACKET_CALLS else "")
        text += f" offered={host[2].tolist()}" if call in MIXED_CALLS else ""
        text += f" status={parts[1].tolist()}" if call in DECODE_CALLS else ""
        return text + f" blocks={parts[0].tolist()} sha={_sha(*parts)}"

    def state(self, kind, h, window=W):
        """The object's visible state and the four last-call records."""
        L = self.L
        if kind == "plain":
            a = [np.zeros(NF, dtype=np.int32) for _ in range(3)]
            total = L.ldpc_amd_fec_rx_flows_pending(h, *(x.ctypes.data for x in a))
            text = f"pending={total} cur={a[0].tolist()} ccnt={a[1].tolist()} ncnt={a[2].tolist()}"
            text += f" dropped={[int(L.ldpc_amd_fec_rx_flows_dropped(h, f)) for f in range(NF)]}"
        else:
            base, cnt = np.zeros(NF, dtype=np.int32), np.zeros((NF, window), dtype=np.int32)
            total = L.ldpc_amd_fec_rxw_flows_pending(h, base.ctypes.data, cnt.ctypes.data)
            stats, ahead, dropped = [], [], []
            for f in range(NF):
                t, b, ah, c = (C.c_int64 * 5)(), C.c_int32(0), C.c_int64(0), np.zeros(window, dtype=np.int32)
                assert L.ldpc_amd_fec_rxw_flows_stats(h, f, t) == 0 and L.ldpc_amd_fec_rxw_flows_state(h, f, C.byref(b), c.ctypes.data, C.byref(ah)) == 0
                assert b.value == base[f] and c.tolist() == cnt[f].tolist()   # the two getters agree
                stats.append([int(v) for v in t]); ahead.append(ah.value); dropped.append(int(L.ldpc_amd_fec_rxw_flows_dropped(h, f)))
            text = f"pending={total} base={base.tolist()} cnt={cnt.tolist()} ahead={ahead} stats={stats} dropped={dropped}"
        text += f" unrouted={int(getattr(L, PRE[kind] + 'unrouted')(h))}"
        return text + " | " + self.infos()

    def infos(self):
        words = []
        for name, ty in (("receiver", C.c_int), ("flows_flush", C.c_int64), ("rxw_flows", C.c_int64), ("flows_demux", C.c_int64)):
            info = (ty * 4)()
            assert getattr(self.L, f"ldpc_amd_fec_{name}_info")(self.ctx._h, info) == 0
            words.append(f"{name}=" + ",".join(str(int(x)) for x in info))
        return " ".join(words)


USABLE = ({0: 0, 2: 0}, {0: 90, 2: 100})   # the packets of the good call behind every case: enough to close blocks and to leave some open


def _usable(env, kind, h, call, name):
    """A good call through `call` (create, destroy: decode_many) on the object of the good calls: its status, its outputs and the
    state it leaves as digests."""
    call = call if call in PACKET_CALLS + FLUSH_CALLS else "decode_many"
    P, fb, _ = env.batch(*USABLE, call in MIXED_CALLS)
    rc, o = env.call(kind, h, call, P, fb, left="dev" if call in MIXED_CALLS else None)
    assert rc >= 0, (name, rc, env.L.ldpc_amd_last_error(env.ctx._h))
    return [int(rc), env.digest(call, rc, o, P, True, short=True) + " state=" + hashlib.sha1(env.state(kind, h).encode()).hexdigest()[:8]]


def _run_cases(envs, rows):
    env = envs[16]
    objs = {}
    for kind in KINDS:   # "": the object of the good calls; s20: S = 20 under symbol unit 16; empty: never fed
        for tag, S in (("", 16), ("s20", 20), ("empty", 16)):
            rc, objs[kind, tag] = env.create(kind, S=S)
            assert rc == 0
        rows.append([f"{kind}: first call", 0, "no error", env.state(kind, objs[kind, ""])] + _usable(env, kind, objs[kind, ""], "decode_many", kind))
    for name, kind, call, kw in CASES:
        kw = dict(kw)
        tag = kw.pop("obj", "")
        before = env.state(kind, objs[kind, tag])
        if call == "create":
            rc, h = env.create(kind, **kw)
            assert rc != 0 and not h.value
        elif call == "destroy":
            env.destroy(kind, None)
            rc = 0
        else:
            P, fb, _ = env.batch(*USABLE, call in MIXED_CALLS)
            if "P" in kw:   # a segmented call's packet count is the end of its flow_begin
                P = kw.pop("P")
                fb = [0, 0, 0, P]
            if "fb" in kw:
                fb = kw.pop("fb")
            rc, _ = env.call(kind, objs[kind, tag], call, P, fb, **kw)
        after = env.state(kind, objs[kind, tag])
        rows.append([name, int(rc), env.L.ldpc_amd_last_error(env.ctx._h).decode() if rc < 0 else "no error", "unchanged" if after == before else after]
                    + _usable(env, kind, objs[kind, ""], call, name))
    for (kind, _), h in objs.items():
        env.destroy(kind, h)


# the good sequences: (name, kind, symbol unit, S, create arguments, packets' offset in their buffer, rx_pkt)
def _good():
    out = []
    for kind in KINDS:
        out.append((f"{kind} S=16", kind, 16, {}, 0, None))
        out.append((f"{kind} S=20 at unit 4", kind, 4, {}, 0, None))
        out.append((f"{kind} S=16, packets 4 bytes off", kind, 16, {}, 4, None))
        out.append((f"{kind} S=16, rx_pkt = 0", kind, 16, {}, 0, 0))
    mds = api.fec_rx_rule_mds
    out.append(("win S=16, depth 2", "win", 16, {"depth": 2}, 0, None))
    out.append(("win S=16, MDS preset", "win", 16, {"rule": lambda: mds(N, K, 1)}, 0, None))
    out.append(("win S=16, depth 2, MDS preset", "win", 16, {"depth": 2, "rule": lambda: mds(N, K, 2)}, 0, None))
    return out


GOOD = _good()
STEPS = (({0: 0, 2: 0}, {0: 20, 2: 25}), ({0: 20, 2: 25}, {0: 200, 2: 290}))   # closes nothing; then more blocks than max_blocks_per_flow


def _run_good(envs, rows):
    for name, kind, unit, ckw, off, rx_pkt in GOOD:
        env = envs[unit]
        ckw = {k: (v() if callable(v) else v) for k, v in ckw.items()}
        if rx_pkt is not None:
            env.ctx.configure("rx_pkt", rx_pkt)
        for mixed in (False, True):
            # the call that closes nothing through one entry point, the call that stops at max_blocks_per_flow through the other
            first, second = ("decode", "push") if mixed else ("push", "decode")
            rc, h = env.create(kind, **ckw)
            assert rc == 0, env.L.ldpc_amd_last_error(env.ctx._h)
            for a, what, (lo, hi) in zip((first, second), ("nothing closes", "stops at max_blocks_per_flow"), STEPS):
                call = f"{a}_{'mixed' if mixed else 'many'}"
                tag = f"good {name}: {call} ({what})"
                P, fb, _ = env.batch(lo, hi, mixed, off)
                rc, o = env.call(kind, h, call, P, fb, packets=("dev", off), left="dev" if mixed else None)
                assert rc >= 0, (tag, rc, env.L.ldpc_amd_last_error(env.ctx._h))
                rows.append([tag, int(rc), env.digest(call, rc, o, P, True), env.state(kind, h)])
            fl = ("decode_flush_many", "flush_many") if mixed else ("flush_many", "decode_flush_many")
            for call, flows in zip(fl, ([2], None)):
                tag = f"good {name}: {call} of {'flow 2' if flows else 'all flows'} after {second}_{'mixed' if mixed else 'many'}"
                rc, o = env.call(kind, h, call, 0, None, flows=flows, rounds=2)
                assert rc >= 0, (tag, rc, env.L.ldpc_amd_last_error(env.ctx._h))
                rows.append([tag, int(rc), env.digest(call, rc, o, 0, False, nsel=1 if flows else NF), env.state(kind, h)])
            env.destroy(kind, h)
        if rx_pkt is not None:
            env.ctx.configure("rx_pkt", 1)   # the shipped default


def run(ctx, ctx4):
    """The table of the library api.load_library() has loaded: the rows the module's text describes."""
    import torch
    assert ctx.symbol_unit() == 16 and ctx4.symbol_unit() == 4
    envs = {16: _Env(ctx, torch, 16), 4: _Env(ctx4, torch, 20)}
    rows = []
    _run_cases(envs, rows)
    _run_good(envs, rows)
    return rows


def contexts():
    import torch
    ctx, ctx4 = api.Context(0), api.Context(0)
    for c in (ctx, ctx4):
        c.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx4.set_symbol_unit(4)
    return ctx, ctx4


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    api.LIB_PATH = os.path.abspath(a.lib)
    ctx, ctx4 = contexts()
    table = run(ctx, ctx4)
    ctx.close()
    ctx4.close()
    with open(a.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in table) + "\n]\n")   # one row per line
    print(len(table), "rows ->", a.out)
