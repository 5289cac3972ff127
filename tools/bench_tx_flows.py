#!/usr/bin/env python3
"""The multi-flow sender (include/ldpc_erasure_amd_sender_flows.h) against what a caller had to do without it, on one GPU: source
frames of many flows in GPU memory -> ONE multiplexed array of FEC wire packets with a flow number per packet, the input of
FecRxFlows.decode_mixed.  BASELINE cfg 2 shape: the (2040,1530) code at S = 1024, 4096 frames in all, split evenly over nflows =
1, 8, 64, 256 streams.

    A   flows    ONE fec_encode_packets_flows_device, ROUND_ROBIN, with flow_of
    B   loop     nflows fec_encode_packets_device calls (one per flow, into its segment), then ONE index_select into the multiplexed
                 order (index and flow_of prepared beforehand, not timed): every payload byte moves twice
    C   single   ONE fec_encode_packets_device over all 4096 frames: the floor, nothing multiplexed
    C2  single   the same call once more in the same steps: the spread of C against itself
    A0  flows    ONE fec_encode_packets_flows_device, SEGMENTED, without flow_of

The variants alternate step by step in ONE process, after a warm-up of each, and are timed with device events around the whole step.
Before timing, A is checked against B (bytes and flow_of) and A0 against C.  Per nflows and variant: median / min / max ms per step;
the ratios A / B (the call's reason to exist: at most 1 from 8 flows on), A / C (recorded) and, at nflows = 1, A0 / C beside C2 / C,
and A0 and C once more as the second of two calls enqueued back to back (two calls minus one call): the call without the host's part.

With --parent-lib PATH (a build of the library from the commit before this feature) the single-flow fused sender of that build is timed
in the same process, twice, around this build's: the existing call must stay within the spread of the two runs of the old build.

    python tools/bench_tx_flows.py [--frames 4096] [--steps 10] [--warmup 2] [--nflows 1,8,64,256] [--parent-lib old.so]
                                   [--out profiles/tx_flows_bench.json]

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def summary(v):
    return {"ms_per_step_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def context_of(api, torch, so=None):
    """A context of the library at `so` (default: this tree's build); two builds live side by side in one process."""
    if so is None:
        ctx = api.Context(0)
    else:
        keep = api._lib, api.LIB_PATH
        api._lib, api.LIB_PATH = None, os.path.abspath(so)
        try:
            ctx = api.Context(0)
        finally:
            api._lib, api.LIB_PATH = keep
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nflows", default="1,8,64,256")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ldpc_erasure_codes_amd import api, codes
    F, S = a.frames, a.S
    ctx = context_of(api, torch)
    h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
    n, k, _ = ctx.code_info(h)
    P = F * n
    src = torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "packets": P, "steps": a.steps,
           "warmup": a.warmup, "knobs": ctx.knobs(), "runs": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out_a = torch.empty((P, 8 + S), dtype=torch.uint8, device="cuda")     # A / A0 / C write here
    out_b = torch.empty((P, 8 + S), dtype=torch.uint8, device="cuda")     # B: the per-flow segments, then ...
    out_m = torch.empty((P, 8 + S), dtype=torch.uint8, device="cuda")     # ... the multiplexed array

    def timed(body):
        torch.cuda.synchronize()
        ev[0].record()
        body()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    for nf in [int(x) for x in a.nflows.split(",")]:
        assert F % nf == 0
        per = F // nf
        fb = np.arange(nf + 1, dtype=np.int64) * per
        cls = (1 + np.arange(nf)) & 0xFF
        blk = (7 * np.arange(nf)) & 0xFF
        # the multiplexed order for B, stated as a sort of the packets by (round, flow): prepared once, not timed
        flow = np.repeat(np.arange(nf), per * n)
        perm_h = np.lexsort((flow, np.tile(np.arange(per * n), nf)))
        perm = torch.from_numpy(perm_h).cuda()
        flow_b = torch.from_numpy(flow[perm_h].astype(np.int32)).cuda()
        got = {}

        def run_a():
            got["A"] = ctx.fec_encode_packets_flows_device(h, src, fb, cls, blk, api.TX_ROUND_ROBIN, out=out_a)

        def run_a0():
            got["A0"] = ctx.fec_encode_packets_flows_device(h, src, fb, cls, blk, api.TX_SEGMENTED, out=out_a, want_flow_of=False)

        def run_b():
            for f in range(nf):
                ctx.fec_encode_packets_device(h, src[f * per:(f + 1) * per], int(cls[f]), int(blk[f]), out=out_b[f * per * n:(f + 1) * per * n])
            torch.index_select(out_b, 0, perm, out=out_m)

        def run_c():
            ctx.fec_encode_packets_device(h, src, int(cls[0]), int(blk[0]), out=out_a)

        # equality before timing: A against B; A0 against the per-flow segments B left in out_b
        run_b()
        run_a()
        torch.cuda.synchronize()
        if not (torch.equal(out_a, out_m) and torch.equal(got["A"][1], flow_b)):
            raise SystemExit(f"nflows = {nf}: the flows call and the loop + index_select differ")
        path_a = ctx.fec_sender_flows_info()["path"]
        run_a0()
        torch.cuda.synchronize()
        if not torch.equal(out_a, out_b):
            raise SystemExit(f"nflows = {nf}: the SEGMENTED flows call and the per-flow calls differ")
        got.clear()
        variants = (("A", run_a), ("B", run_b), ("C", run_c), ("C2", run_c), ("A0", run_a0))
        for _ in range(a.warmup):
            for _, fn in variants:
                timed(fn)
        ms = {nm: [] for nm, _ in variants}
        for _ in range(a.steps):
            for nm, fn in variants:
                ms[nm].append(timed(fn))
        got.clear()
        med = {nm: statistics.median(v) for nm, v in ms.items()}
        run = {"nflows": nf, "frames_per_flow": per, "path": path_a, "variants": {nm: summary(v) for nm, v in ms.items()},
               "A_over_B": round(med["A"] / med["B"], 4), "A_over_C": round(med["A"] / med["C"], 4),
               "A0_over_C": round(med["A0"] / med["C"], 4), "C2_over_C": round(med["C2"] / med["C"], 4)}
        if nf >= 8:
            run["accepted"] = bool(med["A"] <= med["B"])
        else:
            run["A0_within_spread_of_C"] = bool(abs(med["A0"] - med["C"]) <= abs(med["C2"] - med["C"]))
            # where a difference comes from: the second of two calls enqueued back to back has the host's part of the call (for A0
            # the descriptor build and the submission of their copy) hidden behind the first call's kernel
            pair = {}
            for nm, fn in (("C", run_c), ("A0", run_a0)):
                one, two = [], []
                for _ in range(a.steps):
                    one.append(timed(fn))
                    two.append(timed(lambda: (fn(), fn())))
                pair[nm] = round(statistics.median(two) - statistics.median(one), 4)
            run["second_of_two_calls_ms"] = pair
            run["A0_over_C_second_of_two_calls"] = round(pair["A0"] / pair["C"], 4)
            got.clear()
        res["runs"].append(run)
        del perm, flow_b
        torch.cuda.empty_cache()

    if a.parent_lib:
        # the existing single-flow fused sender: the old build, this build, the old build again, alternating step by step
        ctxs = {"parent": context_of(api, torch, a.parent_lib), "this": ctx, "parent_again": context_of(api, torch, a.parent_lib)}
        hs = {nm: (c.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code]) if c is not ctx else h) for nm, c in ctxs.items()}
        ctxs["parent"].fec_encode_packets_device(hs["parent"], src, 1, 0, out=out_b)
        ctx.fec_encode_packets_device(h, src, 1, 0, out=out_a)
        torch.cuda.synchronize()
        if not torch.equal(out_a, out_b):
            raise SystemExit("the single-flow sender of this build and of the parent build differ")
        ms = {nm: [] for nm in ctxs}
        for i in range(a.warmup + a.steps):
            for nm, c in ctxs.items():
                t = timed(lambda: c.fec_encode_packets_device(hs[nm], src, 1, 0, out=out_a))
                if i >= a.warmup:
                    ms[nm].append(t)
        med = {nm: statistics.median(v) for nm, v in ms.items()}
        res["single_flow_sender_vs_parent"] = {
            "paths": {nm: c.fec_sender_info()["path"] for nm, c in ctxs.items()}, "variants": {nm: summary(v) for nm, v in ms.items()},
            "this_over_parent": round(med["this"] / med["parent"], 4), "parent_again_over_parent": round(med["parent_again"] / med["parent"], 4),
            "not_slower_than_the_parent_runs": bool(med["this"] <= max(med["parent"], med["parent_again"]))}
        for nm, c in ctxs.items():
            if c is not ctx:
                c.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
