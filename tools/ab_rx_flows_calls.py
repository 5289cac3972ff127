#!/usr/bin/env python3
"""A/B of two BUILDS of the library on the calls of the two multi-flow device receivers, on one box:
    python tools/ab_rx_flows_calls.py old.so new.so [--rounds 3] [--json-out FILE]
Every round starts one child process per library, alternating (tools/ab_lib.py's scheme).  A child times, for FecRxFlows ("plain")
and FecRxWindowFlows ("win", W = 8, A = 10): decode_many, decode_mixed, push_many and decode_flush_many -- and the windowed
flush_many -- on the (2040,1530) code at S = 1024 and 10 % loss, for every shape of --shapes (frames:flows; BASELINE cfg 2 is
4096:64, and at 16:4 the host work dominates).  Every step runs on a fresh object (a flush on one that an untimed push_many fed the
whole array, which leaves the last blocks of every flow open), device events around the whole call; the child prints the median of
its steps.  Per library: the median of every round, the median over the rounds and the spread between the rounds of the SAME
library -- the yardstick a difference between the libraries has to exceed."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def child(so, shapes, S, steps, warmup):
    import numpy as np
    import torch
    from ldpc_erasure_codes_amd import api, codes
    api.LIB_PATH = so
    from bench_flows import make_packets
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
    n, k, _ = ctx.code_info(h)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {}
    for frames, nf in shapes:
        pk, kept_before = make_packets(torch, ctx, h, n, k, S, frames, 0.10)
        per = frames // nf
        fb = np.ascontiguousarray(kept_before[::per], dtype=np.int64)
        flow_of = torch.from_numpy(np.repeat(np.arange(nf, dtype=np.int32), np.diff(fb))).cuda()
        make = {"plain": lambda: ctx.fec_rx_flows(nf, n, k, S), "win": lambda: ctx.fec_rx_window_flows(nf, n, k, S, 8, 10)}
        calls = {"decode_many": lambda rx: rx.decode_many(h, pk, fb, per), "decode_mixed": lambda rx: rx.decode_mixed(h, pk, flow_of, per),
                 "push_many": lambda rx: rx.push_many(pk, fb, per), "decode_flush_many": lambda rx: rx.decode_flush_many(h),
                 "flush_many": lambda rx: rx.flush_many()}
        for kind in ("plain", "win"):
            for name, fn in calls.items():
                if name == "flush_many" and kind == "plain":
                    continue
                ms = []
                for i in range(warmup + steps):
                    rx = make[kind]()
                    if "flush" in name:
                        rx.push_many(pk, fb, per)
                    torch.cuda.synchronize()
                    ev[0].record()
                    r = fn(rx)
                    ev[1].record()
                    torch.cuda.synchronize()
                    rx.close()
                    if i >= warmup:
                        ms.append(ev[0].elapsed_time(ev[1]))
                    res[f"{kind}_{name}_{frames}x{nf}_blocks"] = int(len(r[1]))
                    del r
                res[f"{kind}_{name}_{frames}x{nf}_ms"] = statistics.median(ms)
        del pk, flow_of
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="4096:64,16:4")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", type=str, default="")
    ap.add_argument("--json-out", type=str, default="")
    a = ap.parse_args()
    if a.child:
        child(a.child, [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")], a.S, a.steps, a.warmup)
        return
    acc = {so: {} for so in a.libs}
    for _ in range(a.rounds):
        for so in a.libs:
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(so), "--shapes", a.shapes, "--S", str(a.S),
                                "--steps", str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True)
            if o.returncode:
                print(o.stderr[-2000:])
                sys.exit(1)
            for kd, v in json.loads(o.stdout.strip().splitlines()[-1]).items():
                acc[so].setdefault(kd, []).append(v)
    out = {"rounds": a.rounds, "shapes": a.shapes, "S": a.S, "steps": a.steps, "libs": {}}
    for so, d in acc.items():
        out["libs"][os.path.basename(os.path.dirname(os.path.abspath(so))) + "/" + os.path.basename(so)] = {
            kd: ({"per_round_ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
                 if kd.endswith("_ms") else v[0]) for kd, v in d.items()}
    print(json.dumps(out))
    if a.json_out:   # one figure per line
        libs = out.pop("libs")
        body = ",\n".join(f' {json.dumps(so)}: {{\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in d.items()) + "\n }" for so, d in libs.items())
        with open(a.json_out, "w") as f:
            f.write(json.dumps(out)[:-1] + ', "libs": {\n' + body + "\n}}\n")


if __name__ == "__main__":
    main()
