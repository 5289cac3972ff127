#!/usr/bin/env python3
"""The multi-flow receiver's batch flush against the loop of per-flow flushes (include/ldpc_erasure_amd_flows_flush.h), on one GPU.
BASELINE cfg 2 shape: the (2040,1530) code at S = 1024; nflows = 8, 64, 256 streams, every one left with TWO open blocks -- a
current block that got 90 % of its packets and a next block that got 20 -- which is what a stream that pauses or ends leaves behind.

    loop    2 nflows FecRxFlows.decode_flush calls, flow by flow (what the library offers without the batch call; this code is
            not touched by the batch flush, so it is the behaviour of the library before it)
    batch   ONE FecRxFlows.decode_flush_many(rounds = 2)
    loop2   the loop a second time: the A/A pair that shows the run's own spread

The variants alternate step by step in ONE process, after a warm-up of each.  Every step refills a fresh flows object (untimed), then
times the drain with a host clock from the first call to the end of a device synchronise behind the last one; the device-event time
of the same window is recorded beside it.  Before timing, the variants' results are checked for equality.  Per nflows and variant:
median / min / max ms per drain; the ratios batch / loop and loop2 / loop of the medians; `batch_below_loop_by_more_than_spread`:
the batch median lies below BOTH loop medians by more than their distance from each other.

    python tools/bench_flows_flush.py [--steps 10] [--warmup 2] [--nflows 8,64,256] [--out profiles/flows_flush_bench.json]

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def flow_packets(torch, ctx, h, n, k, S, part, nxt):
    """One flow's packets, in transmission order: a random `part` of block 0, then the first `nxt` packets of block 1."""
    g = torch.Generator(device="cuda").manual_seed(21)
    src = torch.randint(0, 256, (2, k, S), dtype=torch.uint8, device="cuda", generator=g)
    pk = ctx.fec_packetize_device(ctx.encode(h, src), 1, 0)
    keep = torch.rand(n, device="cuda", generator=g) < part
    return torch.cat([pk[:n][keep], pk[n:n + nxt]]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--part", type=float, default=0.90)
    ap.add_argument("--next", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nflows", default="8,64,256")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ldpc_erasure_codes_amd import api, codes
    S = a.S
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
    n, k, _ = ctx.code_info(h)
    one = flow_packets(torch, ctx, h, n, k, S, a.part, a.next)
    P1 = int(one.shape[0])
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "packets_per_flow": P1, "current_block_part": a.part,
           "next_block_packets": a.next, "steps": a.steps, "warmup": a.warmup, "knobs": ctx.knobs(), "runs": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for nf in [int(x) for x in a.nflows.split(",")]:
        pk = one.repeat(nf, 1)                                 # every flow gets the same packets: the flows do not share state
        fb = np.arange(nf + 1, dtype=np.int64) * P1
        last, info = {}, {}

        def filled():
            rx = ctx.fec_rx_flows(nf, n, k, S)
            closes = rx.push_many(pk, fb, 1)[0]
            assert closes.sum() == 0 and rx.pending().blocks == 2 * nf
            torch.cuda.synchronize()
            return rx

        def timed(nm, drain):
            rx = filled()
            t0 = time.perf_counter()
            ev[0].record()
            last[nm] = drain(rx)
            ev[1].record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rx.close()
            return (t1 - t0) * 1e3, ev[0].elapsed_time(ev[1])

        def loop(nm):
            return timed(nm, lambda rx: [rx.decode_flush(f, h) for f in range(nf) for _ in range(2)])

        def batch(nm):
            r = timed(nm, lambda rx: rx.decode_flush_many(h))
            info[nm] = ctx.fec_flows_flush_info()
            return r

        variants = (("loop", loop), ("batch", batch), ("loop2", loop))
        # the variants give the same blocks and bytes (checked once, on the whole drain)
        loop("loop")
        batch("batch")
        closes, blocks, fr = last["batch"]
        ref = last["loop"]
        ok = len(blocks) == 2 * nf and (closes == 2).all() and np.array_equal(blocks, [r[0] for r in ref])
        for i in range(6):
            ok = ok and torch.equal(fr[i], torch.cat([r[1][i] for r in ref]))
        if not ok:
            raise SystemExit(f"nflows = {nf}: the batch flush and the loop differ")
        del ref, fr
        last.clear()
        torch.cuda.empty_cache()
        for _ in range(a.warmup):
            for nm, fn in variants:
                fn(nm)
                last.clear()
        ms = {nm: [] for nm, _ in variants}
        dev = {nm: [] for nm, _ in variants}
        for _ in range(a.steps):
            for nm, fn in variants:
                w, d = fn(nm)
                ms[nm].append(w)
                dev[nm].append(d)
                last.clear()
        run = {"nflows": nf, "blocks_closed_per_drain": 2 * nf, "batch_info": info["batch"], "variants": {}}
        for nm, v in ms.items():
            run["variants"][nm] = {"ms_per_drain_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                                   "device_event_ms_median": round(statistics.median(dev[nm]), 4)}
        med = {nm: statistics.median(v) for nm, v in ms.items()}
        spread = abs(med["loop2"] - med["loop"])
        run["batch_over_loop"] = round(med["batch"] / med["loop"], 4)
        run["loop2_over_loop"] = round(med["loop2"] / med["loop"], 4)
        run["loop_spread_ms"] = round(spread, 4)
        run["batch_below_loop_by_more_than_spread"] = bool(min(med["loop"], med["loop2"]) - med["batch"] > spread)
        res["runs"].append(run)
        del pk
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
