"""What the five packet senders answer to bad arguments, as a table (tests/test_gpu_sender_refusals.py compares the build under test
with tests/sender_refusals_pinned.json, recorded from the build before the senders' checks were folded into one routine):

    plain      ldpc_amd_fec_encode_packets_dev            flows      ldpc_amd_fec_encode_packets_flows_dev
    ilv        ldpc_amd_fec_encode_packets_ilv_dev        flows_ilv  ldpc_amd_fec_encode_packets_flows_ilv_dev
    rs         ldpc_amd_fec_rs_encode_packets_dev

run(ctx, ctx4) sends every case of CASES through the raw ctypes entry point of its kind and returns rows [name, status, text of
ldpc_amd_last_error]; behind every case a row [name + " / info", 0, the four words of all five ..._info calls], which shows what the
case did to the last-call records; and behind that a good call of the same kind (one frame), whose bytes must be those of the same
call before any case ran: the context is still usable.  (That call sets its kind's record to one frame; the good calls of CASES send
two.)  ctx4: a context at symbol unit 4, for the cases marked unit4.

No case reaches a launch with a bad pointer: every bad pointer is null or host memory, which the library refuses first.

    python tests/sender_refusal_cases.py --lib PATH/libldpc_erasure_amd.so --out FILE     records the table of that build"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ldpc_erasure_codes_amd import api, codes  # noqa: E402

KINDS = ("plain", "flows", "ilv", "flows_ilv", "rs")
LDPC_KINDS = KINDS[:4]
FLOW_KINDS = ("flows", "flows_ilv")
DEPTH_KINDS = ("ilv", "flows_ilv", "rs")
S, F = 16, 2
SRC, PK, FLOW = 0, 1 << 18, 1 << 19   # byte offsets of the three arrays in the device buffer (a call at F = 2, S <= 24 needs 98 KB at most)
BIG = 1 << 31                         # F * n >= 2^31: F = BIG // n + 1


def non_triangular_code():
    """tests/test_gpu_sender.py's: n = 12, k = 6, row r ends at column n - 1 - r, not at k + r -- no systematic encoder."""
    n, k = 12, 6
    H = np.zeros((n - k, n), dtype=np.uint8)
    for r in range(n - k):
        H[r, r] = 1 + r
        H[r, (r + 1) % k] = 7 + r
        H[r, n - 1 - r] = 3
    return codes.from_dense(H, k)


def _cases():
    """(name, kind, unit4, arguments that differ from a good call at F = 2).  Pointers: "dev" (default), "host", None, or
    ("dev" | "host", byte offset from the array's place); for flow_of also "src" / "pk": an address inside that array."""
    out = []

    def add(name, kinds, unit4=False, **kw):
        for kind in kinds:
            a = dict(kw)
            if kind in FLOW_KINDS and a.get("F", "big") != "big":   # the frame count of a multi-flow call is the end of its frame_begin
                nf = a.pop("F")
                a.setdefault("fb", [0, nf] if nf >= 0 else [0, 2, 1])
            out.append((f"{kind}: {name}", kind, unit4, a))

    # the last-call record: a good call of each kind, each kind's call of no frames
    add("good call", KINDS)
    add("no frames", KINDS, F=0)
    add("no frames, null pointers", KINDS, F=0, src=None, pk=None, flow_of=None)
    # single faults
    add("unknown handle", KINDS, handle=999)
    add("S = 0", KINDS, S=0)
    add("S = 24 at unit 16", KINDS, S=24)
    add("negative nframes / decreasing frame_begin", KINDS, F=-1)
    add("frame_begin[0] != 0", FLOW_KINDS, fb=[1, 2, 3])
    add("nflows = 0", FLOW_KINDS, nflows=0)
    add("null frame_begin", FLOW_KINDS, fb=None)
    add("unknown order", FLOW_KINDS, order=7)
    add("depth 3", DEPTH_KINDS, depth=3)
    add("round-robin part group at depth 4", ("flows_ilv",), order=api.TX_ROUND_ROBIN, depth=4)
    add("2^31 packets, null pointers", KINDS, F="big", src=None, pk=None, flow_of=None)
    add("non-triangular code", LDPC_KINDS, handle="nt")
    add("host source", KINDS, src="host")
    add("host packets", KINDS, pk="host")
    add("null source", KINDS, src=None)
    add("host flow_of", FLOW_KINDS, flow_of="host")
    add("misaligned flow_of", FLOW_KINDS, flow_of=("dev", 2))
    add("word-sized S, source at an odd address", KINDS, unit4=True, S=20, src=("dev", 1))
    add("word-sized S, source two bytes off", KINDS, unit4=True, S=20, src=("dev", 2))
    add("word-sized S, aligned (good)", KINDS, unit4=True, S=20)
    add("packets begin inside source", KINDS, pk=("dev", SRC - PK + 64))
    add("source begins inside packets", KINDS, src=("dev", PK - SRC + 64))
    add("flow_of inside packets", FLOW_KINDS, flow_of="pk")
    add("flow_of inside source", FLOW_KINDS, flow_of="src")
    # two faults in one call: which one is reported
    add("unknown handle + S = 0", KINDS, handle=999, S=0)
    add("depth 3 + no frames", DEPTH_KINDS, depth=3, F=0)
    add("S = 24 + no frames", KINDS, S=24, F=0)
    add("2^31 packets + host pointers", KINDS, F="big", src="host", pk="host")
    add("non-triangular code + S = 24", LDPC_KINDS, handle="nt", S=24)
    add("S = 24 + host source", KINDS, S=24, src="host")
    add("host pointers + overlap", KINDS, src="host", pk=("host", SRC - PK + 16), flow_of=None)
    add("host source + flow_of inside packets", FLOW_KINDS, src="host", flow_of="pk")
    add("depth 3 + unknown order", ("flows_ilv",), depth=3, order=7)
    add("S = 0 + nflows = 0", FLOW_KINDS, S=0, nflows=0)
    return out


CASES = _cases()


class _Env:
    """One context's handles and arrays."""

    def __init__(self, ctx, torch):
        self.ctx, self.L, self.torch = ctx, api.load_library(), torch
        self.h = ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
        self.nt = ctx.register_code(non_triangular_code())
        self.rs = ctx.rs_create(15, 11)
        self.dev = torch.zeros(1 << 20, dtype=torch.uint8, device=f"cuda:{ctx.device}")
        self.dev[SRC:PK] = torch.randint(0, 256, (PK - SRC,), dtype=torch.uint8, device=self.dev.device,
                                         generator=torch.Generator(device=self.dev.device).manual_seed(11))
        self.host = np.zeros(1 << 20, dtype=np.uint8)
        self.good = {}

    def nk(self, kind, handle):
        if kind == "rs":
            return 15, 11
        return (12, 6) if handle == "nt" else (2040, 1530)

    def call(self, kind, handle=None, S=S, F=F, fb="two", nflows=None, order=api.TX_SEGMENTED, depth=None, src="dev", pk="dev", flow_of="dev"):
        """fb "two": two flows of one frame each (F frames in one flow where F is "big")."""
        n, _ = self.nk(kind, handle)
        if F == "big":
            F = BIG // n + 1
            fb = [0, F]
        elif fb == "two":
            fb = [0, 1, 2]
        hd = {None: self.rs if kind == "rs" else self.h, "nt": self.nt}.get(handle, handle)

        def ptr(p, place):
            if p is None:
                return None
            where, off = p if isinstance(p, tuple) else (p, 0)
            place = {"src": SRC + 32, "pk": PK + 32}.get(where, place)
            return (self.host.ctypes.data if where == "host" else self.dev.data_ptr()) + place + off
        ps, pp = ptr(src, SRC), ptr(pk, PK)
        if kind in FLOW_KINDS:
            fba = None if fb is None else np.ascontiguousarray(fb, dtype=np.int64)
            nf = (2 if fba is None else fba.shape[0] - 1) if nflows is None else nflows
            cls, blk, pb = np.full(8, 1, dtype=np.uint8), np.zeros(8, dtype=np.uint8), np.zeros(9, dtype=np.int64)
            args = (self.ctx._h, hd, S, nf, None if fba is None else fba.ctypes.data, ps, cls.ctypes.data, blk.ctypes.data, order, pp,
                    ptr(flow_of, FLOW), pb.ctypes.data)
            if kind == "flows":
                return self.L.ldpc_amd_fec_encode_packets_flows_dev(*args)
            return self.L.ldpc_amd_fec_encode_packets_flows_ilv_dev(*args, 2 if depth is None else depth)
        if kind == "plain":
            return self.L.ldpc_amd_fec_encode_packets_dev(self.ctx._h, hd, S, F, ps, 1, 0, pp)
        fn = self.L.ldpc_amd_fec_encode_packets_ilv_dev if kind == "ilv" else self.L.ldpc_amd_fec_rs_encode_packets_dev
        return fn(self.ctx._h, hd, S, F, ps, 1, 0, 2 if depth is None else depth, pp)

    def infos(self):
        words = []
        for name, ty in (("sender", api.C.c_int), ("sender_flows", api.C.c_int64), ("sender_ilv", api.C.c_int64), ("sender_flows_ilv", api.C.c_int64),
                         ("rs_sender", api.C.c_int64)):
            info = (ty * 4)()
            assert getattr(self.L, f"ldpc_amd_fec_{name}_info")(self.ctx._h, info) == 0
            words.append(",".join(str(int(x)) for x in info))
        return " ".join(f"{k}={w}" for k, w in zip(KINDS, words))

    def usable(self, kind):
        """A good call of one frame (for the multi-flow kinds: flow 0's one frame, flow 1 empty): OK, and always the same bytes."""
        self.dev[PK:].fill_(0x5A)
        rc = self.call(kind, F=1, fb=[0, 1, 1])
        self.ctx.synchronize()
        assert rc == 0, (kind, rc, self.L.ldpc_amd_last_error(self.ctx._h))
        got = self.dev[PK:].clone()
        if kind not in self.good:
            n, _ = self.nk(kind, None)
            assert bool((got[n * (8 + S):FLOW - PK] == 0x5A).all()) and not bool((got[:n * (8 + S)] == 0x5A).all())
            self.good[kind] = got
        return bool(self.torch.equal(got, self.good[kind]))


def run(ctx, ctx4):
    """The table of the library api.load_library() has loaded: [[name, status, text], ...]."""
    import torch
    envs = {False: _Env(ctx, torch), True: _Env(ctx4, torch)}
    assert ctx.symbol_unit() == 16 and ctx4.symbol_unit() == 4
    for env in envs.values():
        for kind in KINDS:
            assert env.usable(kind)
    rows = []
    for name, kind, unit4, kw in CASES:
        env = envs[unit4]
        rc = env.call(kind, **kw)
        rows.append([name, int(rc), env.L.ldpc_amd_last_error(env.ctx._h).decode()])
        rows.append([name + " / info", 0, env.infos()])
        env.ctx.synchronize()
        rows.append([name + " / usable", 0, "same bytes" if env.usable(kind) else "OTHER BYTES"])
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
        json.dump(table, f, indent=0)
        f.write("\n")
    print(len(table), "rows ->", a.out)
