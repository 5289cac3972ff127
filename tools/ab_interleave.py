#!/usr/bin/env python3
"""A/B of two BUILDS of the library on the depth-1 paths of the windowed receivers, on one box -- the check that templating the plan
scan on the grouped rule (include/ldpc_erasure_amd_interleave.h) left the plain instantiations alone:
    python tools/ab_interleave.py old.so new.so [--rounds 3] [--json-out profiles/interleave_ab.json]
Every round starts one child process per library, alternating (tools/ab_lib.py's scheme); a child times FecRxWindow.decode_many
(W = 8, A = 10) and FecRxWindowFlows.decode_many (W = 8, A = 10; 1 and 64 flows) on the BASELINE cfg 2 shape -- the (2040,1530) code
at S = 1024, 10 % loss, 4096 frames --, every step on a fresh object, device events around the whole call, and prints the median of
its steps.  Per library: the median of every round, the median over the rounds and the spread between the rounds of the SAME
library.  "verdict": per measurement, the new build's median minus the old build's against the OLD build's own spread -- the bound,
in either direction."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def child(so, frames, S, steps, warmup, flows):
    import numpy as np
    import torch
    from ldpc_erasure_codes_amd import api, codes
    api.LIB_PATH = so
    from bench_flows import make_packets
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
    n, k, _ = ctx.code_info(h)
    pk, kept_before = make_packets(torch, ctx, h, n, k, S, frames, 0.10)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {}

    def timed(make, call):
        ms = []
        for i in range(warmup + steps):
            rx = make()
            torch.cuda.synchronize()
            ev[0].record()
            r = call(rx)
            ev[1].record()
            torch.cuda.synchronize()
            rx.close()
            if i >= warmup:
                ms.append(ev[0].elapsed_time(ev[1]))
        return statistics.median(ms), r

    med, r = timed(lambda: ctx.fec_rx_window(n, k, S, 8, 10), lambda rx: rx.decode_many(h, pk, frames))
    res["rx_window_decode_many_ms"], res["rx_window_blocks"] = med, int(len(r[0]))
    del r
    for nf in flows:
        per = frames // nf
        fb = np.ascontiguousarray(kept_before[::per], dtype=np.int64)
        med, r = timed(lambda: ctx.fec_rx_window_flows(nf, n, k, S, 8, 10), lambda rx: rx.decode_many(h, pk, fb, per))
        res[f"rx_window_flows_{nf}_decode_many_ms"], res[f"rx_window_flows_{nf}_blocks"] = med, int(len(r[1]))
        del r
    ctx.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flows", default="1,64")
    ap.add_argument("--child", type=str, default="")
    ap.add_argument("--json-out", type=str, default="")
    a = ap.parse_args()
    flows = [int(x) for x in a.flows.split(",")]
    if a.child:
        child(a.child, a.frames, a.S, a.steps, a.warmup, flows)
        return
    if len(a.libs) != 2:
        ap.error("two libraries: old.so new.so")
    acc = {so: {} for so in a.libs}
    for _ in range(a.rounds):
        for so in a.libs:
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(so), "--frames", str(a.frames), "--S", str(a.S),
                                "--steps", str(a.steps), "--warmup", str(a.warmup), "--flows", a.flows], capture_output=True, text=True, timeout=600)
            if o.returncode:
                print(o.stderr[-2000:])
                sys.exit(1)
            for kd, v in json.loads(o.stdout.strip().splitlines()[-1]).items():
                acc[so].setdefault(kd, []).append(v)
    out = {"rounds": a.rounds, "frames": a.frames, "S": a.S, "steps": a.steps, "libs": {}, "verdict": {}}
    for tag, so in zip(("old", "new"), a.libs):
        out["libs"][tag] = {kd: ({"per_round_ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4),
                                  "spread_ms": round(max(v) - min(v), 4)} if kd.endswith("_ms") else v[0]) for kd, v in acc[so].items()}
    for kd, o in out["libs"]["old"].items():
        if kd.endswith("_ms"):
            diff = out["libs"]["new"][kd]["median_ms"] - o["median_ms"]
            out["verdict"][kd] = {"new_minus_old_ms": round(diff, 4), "old_spread_ms": o["spread_ms"], "within_spread": bool(abs(diff) <= o["spread_ms"])}
    print(json.dumps(out))
    if a.json_out:
        json.dump(out, open(a.json_out, "w"), indent=1)


if __name__ == "__main__":
    main()
