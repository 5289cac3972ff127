#!/usr/bin/env python3
"""The mixed calls of the windowed multi-flow receiver (include/ldpc_erasure_amd_rx_window_flows_mixed.h) against what a caller had
to do without them, on one GPU: FEC wire packets of many flows INTERLEAVED in GPU memory, a flow number per packet -> decoded
frames.  BASELINE cfg 2 shape: the (2040,1530) code at S = 1024, 10 % uniform loss, 4096 frames in all, split evenly over nflows =
8, 64, 256 streams and interleaved by a random merge (every flow keeps its own order); window W = 8, ahead limit A = 10.

    A  mixed    ONE FecRxWindowFlows.decode_mixed over the interleaved array
    B  sort     torch.argsort(flow_of, stable=True), packets.index_select, a bincount for flow_begin, then
                FecRxWindowFlows.decode_many: the payload bytes move once more
    C  sorted   FecRxWindowFlows.decode_many on packets that were sorted beforehand, the sort not timed: the floor

Two wires per flow count: `merge`, the random merge as it is, and `link`, the same wire passed through FecLink with window 4096
(every packet delayed by up to 4096 packet times: the flows' blocks arrive reordered, which is what the window is for).

The variants alternate step by step in ONE process, after a warm-up of each; every step runs on a fresh object (its per-call scratch
is allocated inside the timed region, in every variant) and is timed with device events around the whole step.  Before timing, the
variants' results are checked for equality.  Per wire, nflows and variant: median / min / max ms per step; the ratios A / B
(mixed_over_sort) and A / C (mixed_over_sorted) of the medians.  Nothing is fixed in advance: the ratios are what is reported.

    python tools/bench_rxw_flows_mixed.py [--frames 4096] [--steps 10] [--warmup 2] [--nflows 8,64,256] [--out profiles/rxw_flows_mixed_bench.json]

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
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--ahead", type=int, default=10)
    ap.add_argument("--link-window", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nflows", default="8,64,256")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench_flows import make_packets
    from ldpc_erasure_codes_amd import api, codes
    F, S, W, A = a.frames, a.S, a.window, a.ahead
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
    n, k, _ = ctx.code_info(h)
    pk, kept_before = make_packets(torch, ctx, h, n, k, S, F, a.loss)       # the flows' segments side by side
    P = int(pk.shape[0])
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "loss": a.loss, "packets": P, "window": W,
           "ahead_limit": A, "link_window": a.link_window, "steps": a.steps, "warmup": a.warmup, "knobs": ctx.knobs(), "runs": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    g = torch.Generator(device="cuda").manual_seed(12)

    def measure(wire, nf, per, mixed, flow_of, srt, fb):
        """The three variants on one wire: `mixed` + flow_of in arrival order, `srt` + fb the same packets sorted by flow."""
        last, paths = {}, {}

        def timed(nm, body):
            rx = ctx.fec_rx_window_flows(nf, n, k, S, W, A)
            torch.cuda.synchronize()
            ev[0].record()
            last[nm] = body(rx)
            ev[1].record()
            torch.cuda.synchronize()
            paths[nm] = ctx.fec_rx_window_flows_info()["path"]
            rx.close()
            return ev[0].elapsed_time(ev[1])

        def sort_then_decode(rx):
            order = torch.argsort(flow_of, stable=True)
            s = mixed.index_select(0, order)
            begin = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.bincount(flow_of, minlength=nf).cumsum(0)]).cpu().numpy()
            return rx.decode_many(h, s, begin, per)

        variants = (("mixed", lambda nm: timed(nm, lambda rx: rx.decode_mixed(h, mixed, flow_of, per)[:4])),
                    ("sort", lambda nm: timed(nm, sort_then_decode)),
                    ("sorted", lambda nm: timed(nm, lambda rx: rx.decode_many(h, srt, fb, per))))
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
                raise SystemExit(f"{wire}, nflows = {nf}: variant {nm} and the sorted call differ")
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
        run = {"wire": wire, "nflows": nf, "frames_per_flow": per, "packets": int(mixed.shape[0]), "blocks_closed_per_step": T, "paths": paths,
               "variants": {}}
        for nm, v in ms.items():
            med = statistics.median(v)
            run["variants"][nm] = {"ms_per_step_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                                   "frames_per_s": round(T / (med * 1e-3), 1)}
        med = {nm: statistics.median(v) for nm, v in ms.items()}
        run["mixed_over_sort"] = round(med["mixed"] / med["sort"], 4)
        run["mixed_over_sorted"] = round(med["mixed"] / med["sorted"], 4)
        res["runs"].append(run)

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
        measure("merge", nf, per, mixed, flow_of, pk, fb)
        # the same wire through the link: reordered within link_window packet times, nothing lost or damaged on top
        arrived, fo, _, _ = ctx.fec_link(100 + nf, window=a.link_window).send(mixed, None, flow_of)
        arrived, fo = arrived.clone(), fo.clone()            # (send returns views of buffers sized for duplicates)
        del mixed, flow_of
        order = torch.argsort(fo, stable=True)
        srt = arrived.index_select(0, order)
        fbl = np.concatenate([[0], np.cumsum(torch.bincount(fo, minlength=nf).cpu().numpy())]).astype(np.int64)
        del order
        torch.cuda.synchronize()
        measure("link", nf, per, arrived, fo, srt, fbl)
        del arrived, fo, srt
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
