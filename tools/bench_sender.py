#!/usr/bin/env python3
"""The device sender, composed against fused (include/ldpc_erasure_amd_sender.h), on one GPU: source symbols in GPU memory ->
FEC wire packets, for the (2040,1530) and the (4080,3060) code at S = 1024.

    composed   ctx.encode into a codeword array, then ctx.fec_packetize_device (what the library offered before the fused call)
    knob0      ctx.fec_encode_packets_device with LDPC_AMD_ENC_PKT=0: the same two kernels through the 256 MiB scratch, in chunks
    fused      ctx.fec_encode_packets_device: the encoder stores the packets itself

The variants alternate step by step in ONE process, after a warm-up of each; every step is timed with device events.  Per variant:
median / min / max ms per step, frames/s, and the algorithmic bytes per second as a share of 8 TB/s -- per frame the composed
paths read k S, write n S, read n S and write n (8 + S); the fused path reads k S and writes n (8 + S).

    python tools/bench_sender.py [--frames 4096] [--steps 20] [--warmup 3] [--out profiles/sender_bench.json]
    python tools/bench_sender.py --only fused --steps 3        (a short run for a rocprofv3 pass)
    python tools/bench_sender.py --merge KEY=FILE.json ...     (adds other measurements' JSON under KEY, no GPU)

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_HBM = 8.0e12   # MI355X HBM3E, bytes/s (datasheet)


def bytes_per_frame(n, k, S):
    return {"composed": k * S + n * S + n * S + n * (S + 8), "fused": k * S + n * (S + 8)}


def run_code(torch, api, codes, code_ind, F, S, steps, warmup, only):
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(code_ind, codes.DEFAULT_COEF_SEED[code_ind])
    n, k, _ = ctx.code_info(h)
    g = torch.Generator(device="cuda").manual_seed(3 + code_ind)
    src = torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=g)
    pk = torch.empty((F * n, 8 + S), dtype=torch.uint8, device="cuda")
    paths = {}

    def composed():
        ctx.fec_packetize_device(ctx.encode(h, src, out=cw), 1, 0, out=pk)

    def knob0():
        ctx.configure("LDPC_AMD_ENC_PKT", 0)
        ctx.fec_encode_packets_device(h, src, 1, 0, out=pk)
        paths["knob0"] = ctx.fec_sender_info()
        ctx.configure("LDPC_AMD_ENC_PKT", None)

    def fused():
        ctx.fec_encode_packets_device(h, src, 1, 0, out=pk)
        paths["fused"] = ctx.fec_sender_info()

    variants = [(nm, fn) for nm, fn in (("composed", composed), ("knob0", knob0), ("fused", fused)) if only in (None, nm)]
    cw = torch.empty((F, n, S), dtype=torch.uint8, device="cuda") if any(nm == "composed" for nm, _ in variants) else None
    knobs_default = ctx.knobs()
    # the variants give the same bytes (checked once, on the whole batch)
    ref = None
    for nm, fn in variants:
        fn()
        torch.cuda.synchronize()
        if ref is None:
            ref = pk.clone()
        elif not torch.equal(pk, ref):
            raise SystemExit(f"{nm}: bytes differ from {variants[0][0]}")
        pk.zero_()
    del ref
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ms = {nm: [] for nm, _ in variants}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(steps):
        for nm, fn in variants:
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[nm].append(ev[0].elapsed_time(ev[1]))
    bpf = bytes_per_frame(n, k, S)
    res = {"code": [n, k], "S": S, "frames": F, "steps": steps, "knobs": knobs_default, "kernel": ctx.profile_kernel_names()["apply"], "variants": {}}
    for nm, v in ms.items():
        med = statistics.median(v)
        b = bpf["fused" if nm == "fused" else "composed"] * F
        res["variants"][nm] = {"ms_per_step_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                               "spread_pct": round(100.0 * (max(v) - min(v)) / med, 2), "frames_per_s": round(F / (med * 1e-3), 1),
                               "algorithmic_bytes_per_step": b, "algorithmic_TBps": round(b / (med * 1e-3) / 1e12, 3),
                               "share_of_8TBps": round(b / (med * 1e-3) / PEAK_HBM, 3), "sender_info": paths.get(nm)}
    if "composed" in ms and "fused" in ms:
        res["composed_over_fused"] = round(statistics.median(ms["composed"]) / statistics.median(ms["fused"]), 3)
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--codes", type=int, nargs="*", default=[1, 3])
    ap.add_argument("--only", choices=("composed", "knob0", "fused"), default=None)
    ap.add_argument("--out")
    ap.add_argument("--merge", nargs="*", default=None, help="KEY=FILE.json: add these to the JSON in --out and exit (no GPU)")
    a = ap.parse_args()
    if a.merge is not None:
        res = json.load(open(a.out))
        for kv in a.merge:
            key, path = kv.split("=", 1)
            res[key] = json.load(open(path))
        json.dump(res, open(a.out, "w"), indent=1)
        return
    import torch
    from ldpc_erasure_codes_amd import api, codes
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_HBM, "runs": []}
    for ci in a.codes:
        res["runs"].append(run_code(torch, api, codes, ci, a.frames, a.S, a.steps, a.warmup, a.only))
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
