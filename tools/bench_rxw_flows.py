#!/usr/bin/env python3
"""The windowed multi-flow receiver (include/ldpc_erasure_amd_rx_window_flows.h) against a loop of single-flow windowed receivers
and against the two-buffer multi-flow receiver, on one GPU: FEC wire packets in GPU memory -> decoded frames, BASELINE cfg 2 shape:
the (2040,1530) code at S = 1024, 10 % uniform loss, packets in transmission order, 4096 frames in all, split evenly over nflows =
1, 8, 64, 256 streams; W = 8, A = 10.

    loop     nflows FecRxWindow.decode_many calls, one object per stream (what the library offered before the flows object: the baseline)
    wflows   ONE FecRxWindowFlows.decode_many over the same packet array, segmented by flow
    flows    ONE FecRxFlows.decode_many (the two-buffer rule) over the same array
    loop2    the loop a second time: the A/A pair that shows the run's own spread

The variants alternate step by step in ONE process, after a warm-up of each; every step runs on fresh receivers (their per-call
scratch is allocated inside the timed region, in every variant) and is timed with device events around the whole step.  Before
timing, wflows and loop are checked for equality.  Per nflows and variant: median / min / max ms per step; the ratios of the medians.
The steps (a)-(e) of one call come from a kernel trace of a short run:

    python tools/bench_rxw_flows.py [--frames 4096] [--steps 10] [--warmup 2] [--nflows 1,8,64,256] [--out profiles/rxw_flows_bench.json]
    rocprofv3 --kernel-trace --stats -d prof_out -- python tools/bench_rxw_flows.py --only wflows --nflows 256 --steps 3

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_flows import make_packets  # noqa: E402

VARIANTS = ("loop", "wflows", "flows", "loop2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--loss", type=float, default=0.10)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--ahead", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nflows", default="1,8,64,256")
    ap.add_argument("--only", choices=VARIANTS, default=None)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ldpc_erasure_codes_amd import api, codes
    F, S, W, A = a.frames, a.S, a.window, a.ahead
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
    n, k, _ = ctx.code_info(h)
    pk, kept_before = make_packets(torch, ctx, h, n, k, S, F, a.loss)
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "loss": a.loss, "packets": int(pk.shape[0]),
           "window": W, "ahead_limit": A, "steps": a.steps, "warmup": a.warmup, "knobs": ctx.knobs(), "runs": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for nf in [int(x) for x in a.nflows.split(",")]:
        assert F % nf == 0
        per = F // nf                                        # frames, and max_blocks, per flow
        fb = np.ascontiguousarray(kept_before[::per], dtype=np.int64)
        assert fb.shape == (nf + 1,) and fb[-1] == pk.shape[0]
        seg = [pk[int(fb[f]):int(fb[f + 1])] for f in range(nf)]
        last, paths = {}, {}

        def timed(rxs, call, info):
            torch.cuda.synchronize()
            ev[0].record()
            r = call()
            ev[1].record()
            torch.cuda.synchronize()
            path = info()["path"]
            for rx in rxs:
                rx.close()
            return r, path, ev[0].elapsed_time(ev[1])

        def loop(nm):
            rxs = [ctx.fec_rx_window(n, k, S, W, A) for _ in range(nf)]
            last[nm], paths[nm], ms = timed(rxs, lambda: [rxs[f].decode_many(h, seg[f], per) for f in range(nf)], ctx.fec_rx_window_info)
            return ms

        def wflows(nm):
            rx = ctx.fec_rx_window_flows(nf, n, k, S, W, A)
            last[nm], paths[nm], ms = timed([rx], lambda: rx.decode_many(h, pk, fb, per), ctx.fec_rx_window_flows_info)
            return ms

        def flows(nm):
            rx = ctx.fec_rx_flows(nf, n, k, S)
            last[nm], paths[nm], ms = timed([rx], lambda: rx.decode_many(h, pk, fb, per), ctx.fec_receiver_info)
            return ms

        variants = [v for v in (("loop", loop), ("wflows", wflows), ("flows", flows), ("loop2", loop)) if a.only in (None, v[0])]
        T = None
        if a.only is None:   # wflows and the loop give the same blocks and bytes (checked once, on the whole batch)
            loop("loop")
            wflows("wflows")
            closes, blocks, fr, consumed = last["wflows"]
            ref = last["loop"]
            ok = (np.array_equal(closes, [len(r[0]) for r in ref]) and np.array_equal(blocks, np.concatenate([r[0] for r in ref])) and
                  np.array_equal(consumed, [r[2] for r in ref]))
            for i in range(6):
                ok = ok and torch.equal(fr[i], torch.cat([r[1][i] for r in ref]))
            if not ok:
                raise SystemExit(f"nflows = {nf}: the windowed flows call and the loop differ")
            T = int(len(blocks))
            del ref, fr
        last.clear()
        torch.cuda.empty_cache()
        for _ in range(a.warmup):
            for nm, fn in variants:
                fn(nm)
                last.clear()
        ms = {nm: [] for nm, _ in variants}
        closed = {}
        for _ in range(a.steps):
            for nm, fn in variants:
                ms[nm].append(fn(nm))
                r = last[nm]
                closed[nm] = int(sum(len(x[0]) for x in r)) if isinstance(r, list) else int(len(r[1]))
                last.clear()
        run = {"nflows": nf, "frames_per_flow": per, "blocks_closed_per_step": T, "paths": paths, "variants": {}}
        for nm, v in ms.items():
            med = statistics.median(v)
            run["variants"][nm] = {"ms_per_step_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                                   "blocks_closed": closed[nm], "frames_per_s": round(closed[nm] / (med * 1e-3), 1)}
        med = {nm: statistics.median(v) for nm, v in ms.items()}
        if "loop" in med:
            for nm in ("wflows", "flows", "loop2"):
                if nm in med:
                    run[nm + "_over_loop"] = round(med[nm] / med["loop"], 4)
        if "wflows" in med and "flows" in med:
            run["wflows_over_flows"] = round(med["wflows"] / med["flows"], 4)
        res["runs"].append(run)
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
