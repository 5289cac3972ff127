#!/usr/bin/env python3
"""The windowed device receiver (include/ldpc_erasure_amd_rx_window.h) against the two-buffer one, on one GPU: FEC wire packets in
GPU memory -> decoded frames, BASELINE cfg 2 shape: the (2040,1530) code at S = 1024, 4096 frames, 10 % uniform loss.

    a        FecRxDevice.decode_many, packets in transmission order                       (the baseline: the existing receiver)
    b        FecRxWindow.decode_many, W = 2, A = 0, the same packets                       (the same rule through the new plan scan)
    c        FecRxWindow.decode_many, W = 8, A = 10, the same packets
    d        FecRxWindow.decode_many, W = 8, A = 10, the same frames through FecLink with window 4096 (two blocks of reordering)
    a_again  a, a second time: the spread of the baseline

The variants alternate step by step in ONE process, after a warm-up of each; every step runs on a fresh receiver and is timed with
device events.  Per variant the median / min / max ms per step; b / a and c / a against the baseline of the same process.  The plan
scan alone (rxw_scan, one wavefront) comes from a kernel trace of a short run:

    python tools/bench_rx_window.py [--frames 4096] [--steps 20] [--warmup 3] [--out profiles/rx_window_bench.json]
    rocprofv3 --kernel-trace --stats -d prof_out -- python tools/bench_rx_window.py --only c --steps 3

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_receiver import make_packets  # noqa: E402

VARIANTS = ("a", "b", "c", "d", "a_again")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--loss", type=float, default=0.10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=VARIANTS, default=None)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from ldpc_erasure_codes_amd import api, codes
    F, S = a.frames, a.S
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
    n, k, _ = ctx.code_info(h)
    pk = make_packets(torch, ctx, h, n, k, S, F, a.loss)
    pk_link = None
    if a.only in (None, "d"):
        pk_link = ctx.fec_link(seed=3, window=4096).send(pk)[0].contiguous()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    info, closes = {}, {}

    def old(name):
        def run():
            rx = ctx.fec_rx_device(n, k, S)
            return rx, lambda: rx.decode_many(h, pk, F)
        return name, run

    def win(name, W, A, packets):
        def run():
            rx = ctx.fec_rx_window(n, k, S, W, A)

            def call():
                r = rx.decode_many(h, packets, F)
                info[name] = dict(ctx.fec_rx_window_info(), stats=rx.stats())
                return r
            return rx, call
        return name, run

    variants = [v for v in (old("a"), win("b", 2, 0, pk), win("c", 8, 10, pk), win("d", 8, 10, pk_link), old("a_again")) if a.only in (None, v[0])]

    def step(run, name, ev=None):
        rx, call = run()   # a fresh receiver: every step sees the stream from its first packet
        torch.cuda.synchronize()
        if ev:
            ev[0].record()
        b, fr, used = call()
        if ev:
            ev[1].record()
        torch.cuda.synchronize()
        closes[name] = (int(len(b)), int(used), int((fr.status.cpu().numpy() <= 1).sum()))
        rx.close()
        return ev[0].elapsed_time(ev[1]) if ev else None

    for _ in range(max(1, a.warmup)):
        for name, run in variants:
            step(run, name)
    ms = {name: [] for name, _ in variants}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(a.steps):
        for name, run in variants:
            ms[name].append(step(run, name, ev))
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "loss": a.loss, "packets": int(pk.shape[0]),
           "packets_through_link": None if pk_link is None else int(pk_link.shape[0]), "steps": a.steps, "knobs": ctx.knobs(), "variants": {}}
    for name, v in ms.items():
        med = statistics.median(v)
        res["variants"][name] = {"ms_per_step_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                                 "blocks_closed": closes[name][0], "packets_consumed": closes[name][1], "frames_recovered": closes[name][2],
                                 "info": info.get(name)}
    if "a" in ms:
        base = statistics.median(ms["a"])
        for name in ("b", "c", "d", "a_again"):
            if name in ms:
                res[name + "_over_a"] = round(statistics.median(ms[name]) / base, 4)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
