#!/usr/bin/env python3
"""The multi-flow device receiver against a loop of single-flow receivers (include/ldpc_erasure_amd_flows.h), on one GPU: FEC
wire packets in GPU memory -> decoded frames, BASELINE cfg 2 shape: the (2040,1530) code at S = 1024, 10 % uniform loss, packets
in transmission order, 4096 frames in all, split evenly over nflows = 1, 8, 64, 256 streams.

    loop    nflows FecRxDevice.decode_many calls, one per stream (what the library offers without the flows object)
    flows   ONE FecRxFlows.decode_many over the same packet array, segmented by flow
    loop2   the loop a second time: the A/A pair that shows the run's own spread

The variants alternate step by step in ONE process, after a warm-up of each; every step runs on fresh receivers (their per-call
scratch is allocated inside the timed region, in every variant) and is timed with device events around the whole step.  Before
timing, the variants' results are checked for equality.  Per nflows and variant: median / min / max ms per step; the ratios
flows / loop and loop2 / loop of the medians.

    python tools/bench_flows.py [--frames 4096] [--steps 10] [--warmup 2] [--nflows 1,8,64,256] [--out profiles/flows_bench.json]

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_packets(torch, ctx, h, n, k, S, F, loss, chunk=512):
    """encode -> packetise chunk by chunk, then the uniform loss.  Returns the packets and, per frame boundary, how many packets
    of the frames before it were kept."""
    g = torch.Generator(device="cuda").manual_seed(11)
    pk = torch.empty((F * n, 8 + S), dtype=torch.uint8, device="cuda")
    for f0 in range(0, F, chunk):
        cnt = min(chunk, F - f0)
        src = torch.randint(0, 256, (cnt, k, S), dtype=torch.uint8, device="cuda", generator=g)
        ctx.fec_packetize_device(ctx.encode(h, src), 1, f0 & 0xFF, out=pk[f0 * n:(f0 + cnt) * n])
    torch.cuda.synchronize()
    keep = torch.rand(F * n, device="cuda", generator=g) >= loss
    out = pk[keep].contiguous()
    kept_before = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), keep.view(F, n).sum(1).cumsum(0)]).cpu().numpy()
    del pk
    torch.cuda.empty_cache()
    return out, kept_before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--loss", type=float, default=0.10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nflows", default="1,8,64,256")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ldpc_erasure_codes_amd import api, codes
    F, S = a.frames, a.S
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
    n, k, _ = ctx.code_info(h)
    pk, kept_before = make_packets(torch, ctx, h, n, k, S, F, a.loss)
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "loss": a.loss, "packets": int(pk.shape[0]),
           "steps": a.steps, "warmup": a.warmup, "knobs": ctx.knobs(), "runs": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for nf in [int(x) for x in a.nflows.split(",")]:
        assert F % nf == 0
        per = F // nf                                        # frames, and max_blocks, per flow
        fb = np.ascontiguousarray(kept_before[::per], dtype=np.int64)
        assert fb.shape == (nf + 1,) and fb[-1] == pk.shape[0]
        seg = [pk[int(fb[f]):int(fb[f + 1])] for f in range(nf)]
        last, paths = {}, {}

        def loop(nm):
            rxs = [ctx.fec_rx_device(n, k, S) for _ in range(nf)]
            torch.cuda.synchronize()
            ev[0].record()
            last[nm] = [rxs[f].decode_many(h, seg[f], per) for f in range(nf)]
            ev[1].record()
            torch.cuda.synchronize()
            paths[nm] = ctx.fec_receiver_info()["path"]
            for rx in rxs:
                rx.close()
            return ev[0].elapsed_time(ev[1])

        def flows(nm):
            rx = ctx.fec_rx_flows(nf, n, k, S)
            torch.cuda.synchronize()
            ev[0].record()
            last[nm] = rx.decode_many(h, pk, fb, per)
            ev[1].record()
            torch.cuda.synchronize()
            paths[nm] = ctx.fec_receiver_info()["path"]
            rx.close()
            return ev[0].elapsed_time(ev[1])

        variants = (("loop", loop), ("flows", flows), ("loop2", loop))
        # the variants give the same blocks and bytes (checked once, on the whole batch)
        loop("loop")
        flows("flows")
        closes, blocks, fr, consumed = last["flows"]
        ref = last["loop"]
        ok = (np.array_equal(closes, [len(r[0]) for r in ref]) and np.array_equal(blocks, np.concatenate([r[0] for r in ref])) and
              np.array_equal(consumed, [r[2] for r in ref]))
        for i in range(6):
            ok = ok and torch.equal(fr[i], torch.cat([r[1][i] for r in ref]))
        if not ok:
            raise SystemExit(f"nflows = {nf}: the flows call and the loop differ")
        T = int(len(blocks))
        del ref, fr
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
        run = {"nflows": nf, "frames_per_flow": per, "blocks_closed_per_step": T, "paths": paths, "variants": {}}
        for nm, v in ms.items():
            med = statistics.median(v)
            run["variants"][nm] = {"ms_per_step_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                                   "frames_per_s": round(T / (med * 1e-3), 1)}
        med = {nm: statistics.median(v) for nm, v in ms.items()}
        run["flows_over_loop"] = round(med["flows"] / med["loop"], 4)
        run["loop2_over_loop"] = round(med["loop2"] / med["loop"], 4)
        res["runs"].append(run)
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
