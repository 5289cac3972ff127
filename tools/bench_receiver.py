#!/usr/bin/env python3
"""The device receiver, composed against fused (include/ldpc_erasure_amd_receiver.h), on one GPU: FEC wire packets in GPU memory
-> decoded frames, BASELINE cfg 2 shape: the (2040,1530) code at S = 1024, 4096 frames, 10 % uniform loss, packets in
transmission order.

    composed   FecRxDevice.push_many into a [B][n][S] array, then ctx.decode_frames (what the library offered before the fused call)
    knob0      FecRxDevice.decode_many with LDPC_AMD_RX_PKT=0: the same kernels through the 256 MiB scratch, in chunks of blocks
    fused      FecRxDevice.decode_many: the decoder fetches its rows from the packets

The variants alternate step by step in ONE process, after a warm-up of each; every step runs on a fresh receiver and is timed
with device events.  Per variant: median / min / max ms per step, frames/s, and the algorithmic bytes per second as a share of
8 TB/s -- per frame the composed paths read the received (1 - loss) n S twice and write n S twice; the fused path reads them
once and writes n S once (headers, flags and row-source words, a few bytes per packet, are left out of both).

    python tools/bench_receiver.py [--frames 4096] [--steps 20] [--warmup 3] [--out profiles/receiver_bench.json]
    python tools/bench_receiver.py --only fused --steps 3        (a short run for a rocprofv3 pass)

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_HBM = 8.0e12   # MI355X HBM3E, bytes/s (datasheet)


def make_packets(torch, ctx, h, n, k, S, F, loss, chunk=512):
    """encode -> packetise chunk by chunk (the codewords of all frames are never held at once), then the uniform loss."""
    g = torch.Generator(device="cuda").manual_seed(11)
    pk = torch.empty((F * n, 8 + S), dtype=torch.uint8, device="cuda")
    for f0 in range(0, F, chunk):
        cnt = min(chunk, F - f0)
        src = torch.randint(0, 256, (cnt, k, S), dtype=torch.uint8, device="cuda", generator=g)
        ctx.fec_packetize_device(ctx.encode(h, src), 1, f0 & 0xFF, out=pk[f0 * n:(f0 + cnt) * n])
    torch.cuda.synchronize()
    keep = torch.rand(F * n, device="cuda", generator=g) >= loss
    out = pk[keep].contiguous()
    del pk
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--loss", type=float, default=0.10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("composed", "knob0", "fused"), default=None)
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
    paths, last = {}, {}

    def composed(rx):
        b, sym, er, used = rx.push_many(pk, F)
        last["composed"] = (b, ctx.decode_frames(h, sym, er), used)

    def knob0(rx):
        ctx.configure("LDPC_AMD_RX_PKT", 0)
        last["knob0"] = rx.decode_many(h, pk, F)
        paths["knob0"] = ctx.fec_receiver_info()
        ctx.configure("LDPC_AMD_RX_PKT", None)

    def fused(rx):
        last["fused"] = rx.decode_many(h, pk, F)
        paths["fused"] = ctx.fec_receiver_info()

    variants = [(nm, fn) for nm, fn in (("composed", composed), ("knob0", knob0), ("fused", fused)) if a.only in (None, nm)]
    knobs_default = ctx.knobs()

    def step(fn, ev=None):
        rx = ctx.fec_rx_device(n, k, S)   # a fresh receiver: every step sees the stream from its first packet
        torch.cuda.synchronize()
        if ev:
            ev[0].record()
        fn(rx)
        if ev:
            ev[1].record()
        torch.cuda.synchronize()
        rx.close()
        return ev[0].elapsed_time(ev[1]) if ev else None

    # the variants give the same blocks and bytes (checked once, on the whole batch)
    ref = None
    for nm, fn in variants:
        step(fn)
        b, fr, used = last[nm]
        if ref is None:
            ref = (b.copy(), [t.clone() for t in fr], used)
            status = fr.status.cpu().numpy()
        elif not (used == ref[2] and (b == ref[0]).all() and all(torch.equal(x, y) for x, y in zip(fr, ref[1]))):
            raise SystemExit(f"{nm}: results differ from {variants[0][0]}")
    closes = int(len(ref[0]))
    del ref
    last.clear()
    torch.cuda.empty_cache()
    for _ in range(a.warmup):
        for _, fn in variants:
            step(fn)
    ms = {nm: [] for nm, _ in variants}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(a.steps):
        for nm, fn in variants:
            ms[nm].append(step(fn, ev))
            last.clear()
    recv = float(pk.shape[0]) / (F * n)
    bpf = {"composed": 2 * (recv + 1.0) * n * S, "fused": (recv + 1.0) * n * S}
    names = ctx.profile_kernel_names()
    res = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_HBM, "code": [n, k], "S": S, "frames": F, "loss": a.loss,
           "packets": int(pk.shape[0]), "blocks_closed_per_step": closes, "frames_decoded_by_message_passing": int((status == 0).sum()),
           "steps": a.steps, "knobs": knobs_default, "kernel": names["apply"], "kernel_tier2": names["apply_tier2"], "variants": {}}
    for nm, v in ms.items():
        med = statistics.median(v)
        by = bpf["fused" if nm == "fused" else "composed"] * closes
        res["variants"][nm] = {"ms_per_step_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                               "spread_pct": round(100.0 * (max(v) - min(v)) / med, 2), "frames_per_s": round(closes / (med * 1e-3), 1),
                               "algorithmic_bytes_per_step": int(by), "algorithmic_TBps": round(by / (med * 1e-3) / 1e12, 3),
                               "share_of_8TBps": round(by / (med * 1e-3) / PEAK_HBM, 3), "receiver_info": paths.get(nm)}
    if "composed" in ms and "fused" in ms:
        res["fused_over_composed"] = round(statistics.median(ms["fused"]) / statistics.median(ms["composed"]), 3)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
