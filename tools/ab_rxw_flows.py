#!/usr/bin/env python3
"""A/B of two BUILDS of the library on the segmented call of the windowed multi-flow receiver, on one box:
    python tools/ab_rxw_flows.py old.so new.so [--rounds 3] [--json-out FILE]
Every round starts one child process per library, alternating (tools/ab_lib.py's scheme); a child times
FecRxWindowFlows.decode_many on the BASELINE cfg 2 shape -- the (2040,1530) code at S = 1024, 10 % loss, 4096 frames, W = 8,
A = 10 -- split over 1 and over 64 flows, every step on a fresh object, device events around the whole call, and prints the median
of its steps.  Per library: the median of every round, the median over the rounds and the spread between the rounds of the SAME
library -- the yardstick a difference between the libraries has to exceed.  --sender-flows 8,64 also times the multi-flow sender
(Context.fec_encode_packets_flows_device, round robin, the same frames split over that many flows) in every child."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def child(so, frames, S, steps, warmup, flows, sender_flows=()):
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
    for nf in flows:
        per = frames // nf
        fb = np.ascontiguousarray(kept_before[::per], dtype=np.int64)
        ms = []
        for i in range(warmup + steps):
            rx = ctx.fec_rx_window_flows(nf, n, k, S, 8, 10)
            torch.cuda.synchronize()
            ev[0].record()
            r = rx.decode_many(h, pk, fb, per)
            ev[1].record()
            torch.cuda.synchronize()
            rx.close()
            if i >= warmup:
                ms.append(ev[0].elapsed_time(ev[1]))
            res[f"blocks_{nf}"] = int(len(r[1]))
            del r
        res[f"decode_many_{nf}_flows_ms"] = statistics.median(ms)
    if sender_flows:
        del pk
        torch.cuda.empty_cache()
        src = torch.randint(0, 256, (frames, k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        out = torch.empty((frames * n, 8 + S), dtype=torch.uint8, device="cuda")
    for nf in sender_flows:
        fb = np.arange(nf + 1, dtype=np.int64) * (frames // nf)
        ms = []
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            ev[0].record()
            ctx.fec_encode_packets_flows_device(h, src, fb, 1, 0, api.TX_ROUND_ROBIN, out=out, want_flow_of=False)
            ev[1].record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms.append(ev[0].elapsed_time(ev[1]))
        res[f"encode_flows_{nf}_flows_ms"] = statistics.median(ms)
        res[f"encode_flows_{nf}_path"] = ctx.fec_sender_flows_info()["path"]
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
    ap.add_argument("--sender-flows", default="")
    ap.add_argument("--child", type=str, default="")
    ap.add_argument("--json-out", type=str, default="")
    a = ap.parse_args()
    flows = [int(x) for x in a.flows.split(",")]
    if a.child:
        child(a.child, a.frames, a.S, a.steps, a.warmup, flows, [int(x) for x in a.sender_flows.split(",") if x])
        return
    acc = {so: {} for so in a.libs}
    for _ in range(a.rounds):
        for so in a.libs:
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(so), "--frames", str(a.frames), "--S", str(a.S),
                                "--steps", str(a.steps), "--warmup", str(a.warmup), "--flows", a.flows, "--sender-flows", a.sender_flows],
                               capture_output=True, text=True)
            if o.returncode:
                print(o.stderr[-2000:])
                sys.exit(1)
            for kd, v in json.loads(o.stdout.strip().splitlines()[-1]).items():
                acc[so].setdefault(kd, []).append(v)
    out = {"rounds": a.rounds, "frames": a.frames, "S": a.S, "steps": a.steps, "libs": {}}
    for so, d in acc.items():
        out["libs"][os.path.basename(os.path.dirname(os.path.abspath(so))) + "/" + os.path.basename(so)] = {
            kd: ({"per_round_ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
                 if kd.endswith("_ms") else v[0]) for kd, v in d.items()}
    print(json.dumps(out))
    if a.json_out:
        json.dump(out, open(a.json_out, "w"), indent=1)


if __name__ == "__main__":
    main()
