#!/usr/bin/env python3
"""A/B of two BUILDS of the library on the five packet senders, on one box -- the check that folding their host code left the
per-call host work alone (the device code of the two builds is the same):
    python tools/ab_senders.py old.so new.so [--rounds 3] [--json-out profiles/tx_refactor_ab.json]
Every round starts one child process per library, alternating (tools/ab_lib.py's scheme); a child times the five sender calls whole,
device events around the call, on the BASELINE cfg 2 shape -- the (2040,1530) code at S = 1024, 4096 frames; 64 flows for the
multi-flow senders, depth 8 for the depth senders, RS(255,192) for the RS sender -- and on a small call (16 frames), where the host
work dominates, and prints the median of its steps.  Per library: the median of every round, the median over the rounds and the
spread between the rounds of the SAME library.  "verdict": per measurement, the new build's median minus the old build's against the
OLD build's own spread -- the bound, in either direction."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(so, frames, small, S, steps, warmup, nflows, depth):
    import numpy as np
    import torch
    from ldpc_erasure_codes_amd import api, codes
    api.LIB_PATH = so
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
    n, k, _ = ctx.code_info(h)
    rs = ctx.rs_create(255, 192)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {}

    def timed(call):
        ms = []
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            ev[0].record()
            call()
            ev[1].record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms.append(ev[0].elapsed_time(ev[1]))
        return statistics.median(ms)

    for tag, F in (("", frames), ("_small", small)):
        gen = torch.Generator(device="cuda").manual_seed(F)
        src = torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=gen)
        out = torch.empty((F * n, 8 + S), dtype=torch.uint8, device="cuda")
        nf = min(nflows, F // depth)
        fb = np.arange(nf + 1, dtype=np.int64) * (F // nf)
        res[f"plain{tag}_ms"] = timed(lambda: ctx.fec_encode_packets_device(h, src, 1, 0, out=out))
        res[f"flows{tag}_ms"] = timed(lambda: ctx.fec_encode_packets_flows_device(h, src, fb, 1, 0, api.TX_ROUND_ROBIN, out=out))
        res[f"ilv{tag}_ms"] = timed(lambda: ctx.fec_encode_packets_interleaved_device(h, src, depth, 1, 0, out=out))
        res[f"flows_ilv{tag}_ms"] = timed(lambda: ctx.fec_encode_packets_flows_interleaved_device(h, src, fb, 1, 0, api.TX_ROUND_ROBIN, depth, out=out))
        res[f"paths{tag}"] = [ctx.fec_sender_info()["path"], ctx.fec_sender_flows_info()["path"], ctx.fec_sender_ilv_info()["path"],
                              ctx.fec_sender_flows_ilv_info()["path"]]
        del src, out
        rsrc = torch.randint(0, 256, (F, 192, S), dtype=torch.uint8, device="cuda", generator=gen)
        rout = torch.empty((F * 255, 8 + S), dtype=torch.uint8, device="cuda")
        res[f"rs{tag}_ms"] = timed(lambda: ctx.fec_rs_encode_packets_device(rs, rsrc, depth, out=rout))
        res[f"paths{tag}"].append(ctx.fec_rs_sender_info()["path"])
        del rsrc, rout
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--small", type=int, default=16)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flows", type=int, default=64)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--child", type=str, default="")
    ap.add_argument("--json-out", type=str, default="")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.frames, a.small, a.S, a.steps, a.warmup, a.flows, a.depth)
        return
    if len(a.libs) != 2:
        ap.error("two libraries: old.so new.so")
    acc = {so: {} for so in a.libs}
    for _ in range(a.rounds):
        for so in a.libs:
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(so), "--frames", str(a.frames), "--small", str(a.small),
                                "--S", str(a.S), "--steps", str(a.steps), "--warmup", str(a.warmup), "--flows", str(a.flows), "--depth", str(a.depth)],
                               capture_output=True, text=True, timeout=300)
            if o.returncode:
                print(o.stderr[-2000:])
                sys.exit(1)
            for kd, v in json.loads(o.stdout.strip().splitlines()[-1]).items():
                acc[so].setdefault(kd, []).append(v)
    out = {"rounds": a.rounds, "frames": a.frames, "small_frames": a.small, "S": a.S, "steps": a.steps, "flows": a.flows, "depth": a.depth,
           "libs": {}, "verdict": {}}
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
