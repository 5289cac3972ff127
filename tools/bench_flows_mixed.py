#!/usr/bin/env python3
"""The mixed calls of the multi-flow receiver (include/ldpc_erasure_amd_flows_mixed.h) against what a caller had to do without
them, on one GPU: FEC wire packets of many flows INTERLEAVED in GPU memory, a flow number per packet -> decoded frames.  BASELINE
cfg 2 shape: the (2040,1530) code at S = 1024, 10 % uniform loss, 4096 frames in all, split evenly over nflows = 8, 64, 256 streams
and interleaved by a random merge (every flow keeps its own order).

    A  mixed    ONE FecRxFlows.decode_mixed over the interleaved array
    B  sort     torch.argsort(flow_of, stable=True), packets.index_select, a bincount for flow_begin, then FecRxFlows.decode_many:
                the payload bytes move once more
    C  sorted   FecRxFlows.decode_many on packets that were sorted beforehand, the sort not timed: the floor

The variants alternate step by step in ONE process, after a warm-up of each; every step runs on a fresh object (its per-call
scratch is allocated inside the timed region, in every variant) and is timed with device events around the whole step.  Before
timing, the variants' results are checked for equality.  Per nflows and variant: median / min / max ms per step; the ratios A / B
(acceptance: at most 1) and A / C of the medians; and the partition alone (ldpc_amd_fec_flows_demux_dev, synchronous) in packets/s.

    python tools/bench_flows_mixed.py [--frames 4096] [--steps 10] [--warmup 2] [--nflows 8,64,256] [--out profiles/flows_mixed_bench.json]

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--loss", type=float, default=0.10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nflows", default="8,64,256")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench_flows import make_packets
    from ldpc_erasure_codes_amd import api, codes
    F, S = a.frames, a.S
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
    n, k, _ = ctx.code_info(h)
    pk, kept_before = make_packets(torch, ctx, h, n, k, S, F, a.loss)       # the flows' segments side by side: variant C's input
    P = int(pk.shape[0])
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "loss": a.loss, "packets": P,
           "steps": a.steps, "warmup": a.warmup, "knobs": ctx.knobs(), "runs": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    g = torch.Generator(device="cuda").manual_seed(12)
    for nf in [int(x) for x in a.nflows.split(",")]:
        assert F % nf == 0
        per = F // nf                                        # frames, and max_blocks, per flow
        fb = np.ascontiguousarray(kept_before[::per], dtype=np.int64)
        assert fb.shape == (nf + 1,) and fb[-1] == P
        # a random merge: a random arrangement of the flow numbers; the q-th packet of the sorted array goes where its number's turn is
        sorted_ids = torch.repeat_interleave(torch.arange(nf, dtype=torch.int32, device="cuda"), torch.from_numpy(np.diff(fb)).cuda())
        flow_of = sorted_ids[torch.randperm(P, device="cuda", generator=g)].contiguous()
        where = torch.argsort(flow_of, stable=True)
        mixed = torch.empty_like(pk)
        mixed[where] = pk
        del where, sorted_ids
        torch.cuda.synchronize()
        last, paths = {}, {}

        def timed(nm, body):
            rx = ctx.fec_rx_flows(nf, n, k, S)
            torch.cuda.synchronize()
            ev[0].record()
            last[nm] = body(rx)
            ev[1].record()
            torch.cuda.synchronize()
            paths[nm] = ctx.fec_receiver_info()["path"]
            rx.close()
            return ev[0].elapsed_time(ev[1])

        def sort_then_decode(rx):
            order = torch.argsort(flow_of, stable=True)
            srt = mixed.index_select(0, order)
            begin = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.bincount(flow_of, minlength=nf).cumsum(0)]).cpu().numpy()
            return rx.decode_many(h, srt, begin, per)

        variants = (("mixed", lambda nm: timed(nm, lambda rx: rx.decode_mixed(h, mixed, flow_of, per)[:4])),
                    ("sort", lambda nm: timed(nm, sort_then_decode)),
                    ("sorted", lambda nm: timed(nm, lambda rx: rx.decode_many(h, pk, fb, per))))
        # the variants give the same blocks and bytes (checked once, on the whole batch)
        for nm, fn in variants:
            fn(nm)
        closes, blocks, fr, consumed = last["sorted"]
        for nm in ("mixed", "sort"):
            c2, b2, fr2, u2 = last[nm]
            ok = np.array_equal(closes, c2) and np.array_equal(blocks, b2) and np.array_equal(consumed, u2)
            for i in range(6):
                ok = ok and torch.equal(fr[i], fr2[i])
            if not ok:
                raise SystemExit(f"nflows = {nf}: variant {nm} and the sorted call differ")
        T = int(len(blocks))
        del fr, fr2
        last.clear()
        torch.cuda.empty_cache()
        for _ in range(a.warmup):
            for nm, fn in variants:
                fn(nm)
                last.clear()
        ms = {nm: [] for nm, _ in variants}
        for _ in range(a.steps):
            for nm, fn in variants:
                ms[nm].append(fn(nm))
                last.clear()
        # the partition alone
        order = torch.empty(P, dtype=torch.int32, device="cuda")
        part = []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            ev[0].record()
            R = ctx._L.ldpc_amd_fec_flows_demux_dev(ctx._h, flow_of.data_ptr(), P, nf, order.data_ptr(), None)
            ev[1].record()
            torch.cuda.synchronize()
            assert R == P
            if i >= a.warmup:
                part.append(ev[0].elapsed_time(ev[1]))
        run = {"nflows": nf, "frames_per_flow": per, "blocks_closed_per_step": T, "paths": paths, "variants": {},
               "demux_info": ctx.fec_flows_demux_info()}
        for nm, v in ms.items():
            med = statistics.median(v)
            run["variants"][nm] = {"ms_per_step_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                                   "frames_per_s": round(T / (med * 1e-3), 1)}
        med = {nm: statistics.median(v) for nm, v in ms.items()}
        run["mixed_over_sort"] = round(med["mixed"] / med["sort"], 4)
        run["mixed_over_sorted"] = round(med["mixed"] / med["sorted"], 4)
        run["accepted"] = bool(med["mixed"] <= med["sort"])
        pm = statistics.median(part)
        run["partition_only"] = {"ms_median": round(pm, 4), "packets_per_s": round(P / (pm * 1e-3), 1)}
        res["runs"].append(run)
        del mixed, flow_of, order
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
