#!/usr/bin/env python3
"""The block-interleaved wire (include/ldpc_erasure_amd_interleave.h) on one GPU, BASELINE shape: the (2040,1530) code at S = 1024,
4096 frames.

    sender    Context.fec_encode_packets_interleaved_device at depth 1 / 4 / 8 / 16 against Context.fec_encode_packets_device, the
              variants alternating step by step in one process, device events around every call
    receiver  FecRxWindow(W = 16, A = 10, depth = 8).decode_many on the depth-8 wire against FecRxWindow(W = 16, A = 10).decode_many
              on the straight wire, 10 % uniform loss on both, every step on a fresh object
    quality   blocks decoded (status <= 1) of the 4096 sent at depth 1 / 4 / 8 / 16: sender -> FecLink (no reordering, the
              Gilbert-Elliott loss of BASELINE cfg 3 by wire position) -> FecRxWindow(W = 2 * depth, at least 16; A = 10).decode_many
              + decode_flush

    python tools/bench_interleave.py [--frames 4096] [--steps 10] [--warmup 2] [--out profiles/interleave_bench.json]

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GE_PARAMS = (0.13, 0.8, 10.0)   # bench.py's cfg 3 channel: alpha, beta, good_transition_bias
DEPTHS = (1, 4, 8, 16)


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--loss", type=float, default=0.10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from ldpc_erasure_codes_amd import api, codes
    F, S = a.frames, a.S
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
    n, k, _ = ctx.code_info(h)
    g = torch.Generator(device="cuda").manual_seed(11)
    src = torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty((F * n, 8 + S), dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "steps": a.steps, "knobs": ctx.knobs()}

    # ---- sender
    def straight():
        ctx.fec_encode_packets_device(h, src, 1, 0, out=out)

    def deep(D):
        return lambda: ctx.fec_encode_packets_interleaved_device(h, src, D, 1, 0, out=out)

    senders = [("straight", straight)] + [("depth_%d" % D, deep(D)) for D in DEPTHS] + [("straight_again", straight)]
    ms = {name: [] for name, _ in senders}
    for i in range(a.warmup + a.steps):
        for name, fn in senders:
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[name].append(ev[0].elapsed_time(ev[1]))
    res["sender"] = {name: stats(v) for name, v in ms.items()}
    res["sender"]["path"] = ctx.fec_sender_ilv_info()["path"]
    base = statistics.median(ms["straight"])
    for name in ms:
        if name != "straight":
            res["sender"][name]["over_straight"] = round(statistics.median(ms[name]) / base, 4)

    # ---- receiver: the same uniform loss pattern on the straight and on the depth-8 wire
    keep = torch.rand(F * n, device="cuda", generator=g) >= a.loss
    wires = {}
    for name, D in (("plain_on_straight", 1), ("depth_8_on_interleaved", 8)):
        ctx.fec_encode_packets_interleaved_device(h, src, D, 1, 0, out=out)
        torch.cuda.synchronize()
        wires[name] = (out[keep].contiguous(), D)
    ms = {name: [] for name in wires}
    got = {}
    for i in range(a.warmup + a.steps):
        for name, (pk, D) in wires.items():
            rx = ctx.fec_rx_window(n, k, S, 16, 10, depth=D)
            torch.cuda.synchronize()
            ev[0].record()
            b, fr, used = rx.decode_many(h, pk, F)
            ev[1].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[name].append(ev[0].elapsed_time(ev[1]))
            got[name] = {"blocks_closed": int(len(b)), "packets_consumed": int(used), "frames_decoded": int((fr.status.cpu().numpy() <= 1).sum()),
                         "totals": rx.stats(), "path": ctx.fec_rx_window_info()["path"]}
            rx.close()
            del b, fr
    res["receiver"] = {name: dict(stats(v), packets=int(wires[name][0].shape[0]), **got[name]) for name, v in ms.items()}
    res["receiver"]["depth_8_over_plain"] = round(statistics.median(ms["depth_8_on_interleaved"]) / statistics.median(ms["plain_on_straight"]), 4)
    del wires
    torch.cuda.empty_cache()

    # ---- quality: the cfg 3 Gilbert-Elliott loss by wire position, no reordering
    lost = torch.empty(F * n, dtype=torch.uint8, device="cuda")
    ctx.synth_erasures_bursty(79, 0, F * n, 1, *GE_PARAMS, lost)
    res["quality"] = {"channel": {"alpha": GE_PARAMS[0], "beta": GE_PARAMS[1], "good_transition_bias": GE_PARAMS[2], "seed": 79},
                      "lost_fraction": round(float(lost.float().mean().item()), 5)}
    for D in DEPTHS:
        W = max(16, 2 * D)
        ctx.fec_encode_packets_interleaved_device(h, src, D, 1, 0, out=out)
        arrived = ctx.fec_link(seed=5, window=0).send(out, lost=lost)[0]
        with ctx.fec_rx_window(n, k, S, W, 10, depth=D) as rx:
            ok = closed = 0
            pos = 0
            while pos < arrived.shape[0]:
                b, fr, used = rx.decode_many(h, arrived[pos:], 1024)
                ok += int((fr.status.cpu().numpy() <= 1).sum()) if len(b) else 0
                closed += len(b)
                pos += used
            b, fr = rx.decode_flush(h)
            ok += int((fr.status.cpu().numpy() <= 1).sum()) if len(b) else 0
            closed += len(b)
            res["quality"]["depth_%d" % D] = {"window": W, "blocks_decoded": ok, "blocks_handed_out": closed, "blocks_sent": F, "totals": rx.stats()}
        del arrived
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
