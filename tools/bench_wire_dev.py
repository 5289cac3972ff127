#!/usr/bin/env python3
"""Rates of the device-resident wire path (include/ldpc_erasure_amd_wire_dev.h) on one GPU, cfg 2's (2040,1530) code with
1 KB packets, 10 % loss, re-ordering window 300 -- next to the host reassembler (csrc/wire.cpp) on the same stream:

    packetiser     GB/s (reads n*S, writes n*(8+S) per frame; device events around one launch) and share of 8 TB/s
    reassembler    packets/s of push_many on the device (plan + data movement, wall clock with a synchronise)
    end to end     packets -> decoded frames/s: push_many + decode of each batch, all on the device
    host           packets/s of ldpc_amd_fec_rx_push_many on one core, same stream

The per-kernel rates (plan scan packets/s, gather GB/s) come from a `rocprofv3 --kernel-trace --stats --output-format csv` pass of
this script with --counts FILE, then `--kernel-stats STATS_CSV --counts FILE` (no GPU needed) divides the bytes and packets that pass moved by
the kernels' total durations.  One JSON line on stdout."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_HBM = 8.0e12   # MI355X HBM3E, bytes/s (datasheet)


def kernel_rates(stats_csv, counts):
    tot = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            for key in ("fec_packetize_v16", "fec_rx_headers", "fec_rx_scan", "fec_rx_winners", "fec_rx_move<true", "fec_rx_move<false"):
                if key in row["Name"]:
                    tot[key] = tot.get(key, 0) + int(row["TotalDurationNs"])
    s = lambda k: tot.get(k, 0) * 1e-9   # noqa: E731
    out = {"kernel_seconds": {k: round(v * 1e-9, 6) for k, v in tot.items()}}
    if s("fec_packetize_v16"):
        out["packetize_GBps"] = round(counts["packetize_bytes"] / s("fec_packetize_v16") / 1e9, 1)
        out["packetize_peak_fraction"] = round(counts["packetize_bytes"] / s("fec_packetize_v16") / PEAK_HBM, 3)
    if s("fec_rx_scan"):
        out["scan_Mpackets_per_s"] = round(counts["scan_packets"] / s("fec_rx_scan") / 1e6, 1)
        out["headers_scan_Mpackets_per_s"] = round(counts["scan_packets"] / (s("fec_rx_scan") + s("fec_rx_headers")) / 1e6, 1)
    if s("fec_rx_move<true"):
        out["gather_GBps"] = round(counts["gather_bytes"] / s("fec_rx_move<true") / 1e9, 1)
        out["gather_peak_fraction"] = round(counts["gather_bytes"] / s("fec_rx_move<true") / PEAK_HBM, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="max_blocks per push_many of the end-to-end loop")
    ap.add_argument("--counts", help="write (or, with --kernel-stats, read) the bytes / packets the kernels moved")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel_stats.csv of a run of this script: print per-kernel rates, no GPU")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_rates(a.kernel_stats, json.load(open(a.counts)))))
        return

    import torch
    from ldpc_erasure_codes_amd import api, codes
    n, k, S, F = 2040, 1530, 1024, a.frames
    counts = {"packetize_bytes": 0, "scan_packets": 0, "gather_bytes": 0}
    res = {"workload": f"({n},{k}) S={S}, {F} frames, 10% loss, re-order window 300", "device": torch.cuda.get_device_name(0)}
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
    g = torch.Generator(device="cuda").manual_seed(3)
    src = torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=g)
    cw = ctx.encode(h, src)
    pk = torch.empty((F * n, 8 + S), dtype=torch.uint8, device="cuda")

    # packetiser
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = 1e9
    for r in range(a.reps + 1):
        ev[0].record()
        ctx.fec_packetize_device(cw, 1, 0, out=pk)
        ev[1].record()
        torch.cuda.synchronize()
        if r:
            best = min(best, ev[0].elapsed_time(ev[1]) * 1e-3)
        counts["packetize_bytes"] += F * n * (2 * S + 8)
    pbytes = F * n * (2 * S + 8)
    res["packetize_GBps_events"] = round(pbytes / best / 1e9, 1)
    res["packetize_peak_fraction_events"] = round(pbytes / best / PEAK_HBM, 3)

    # channel: 10 % loss, every packet moves up to 300 places (tools/bench_wire.py's stream, built on the device)
    keep = torch.nonzero(torch.rand(F * n, device="cuda", generator=g) >= 0.10).squeeze(1)
    order = keep[torch.argsort(keep.double() + torch.randint(0, 300, keep.shape, device="cuda", generator=g).double())]
    stream = pk[order].contiguous()
    del pk
    P = stream.shape[0]
    res["packets"] = P

    def push(rx, pkts, mb):
        b, sym, er, used = rx.push_many(pkts, mb)
        counts["scan_packets"] += used
        counts["gather_bytes"] += len(b) * n * (2 * S + 2)   # payload read + written, flag read + written
        return b, sym, er, used

    # device reassembler: the whole stream in one call
    best = 1e9
    for r in range(a.reps + 1):
        rx = ctx.fec_rx_device(n, k, S)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b, sym, er, used = push(rx, stream, F)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rx.close()
        if r:
            best = min(best, dt)
        del sym, er
    res["rx_device_Mpackets_per_s"] = round(used / best / 1e6, 1)
    res["rx_device_blocks_closed"] = int(len(b))

    # end to end: packets -> decoded frames, batches of a.batch blocks
    best, frames_done = 1e9, 0
    for r in range(max(2, a.reps // 2 + 1)):
        rx = ctx.fec_rx_device(n, k, S)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pos, frames_done = 0, 0
        while pos < P:
            b, sym, er, used = push(rx, stream[pos:], a.batch)
            pos += used
            if len(b):
                ctx.decode(h, sym, er)
                frames_done += len(b)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rx.close()
        if r:
            best = min(best, dt)
    res["e2e_frames_per_s"] = round(frames_done / best, 1)
    res["e2e_Mpackets_per_s"] = round(P / best / 1e6, 2)
    res["e2e_frames"] = frames_done

    # host reassembler on the same stream, one core
    host = stream.cpu().numpy()
    L = api.load_library()
    hrx = api.FecRx(n, k, S)
    hs = np.ones((F, n, S), dtype=np.uint8)
    he = np.ones((F, n), dtype=np.uint8)
    hb = np.zeros(F, dtype=np.int32)
    used_c = C.c_long(0)
    t0 = time.perf_counter()
    L.ldpc_amd_fec_rx_push_many(hrx._h, host.ctypes.data, P, hs.ctypes.data, he.ctypes.data, hb.ctypes.data, F, C.byref(used_c))
    dt = time.perf_counter() - t0
    hrx.close()
    res["rx_host_Mpackets_per_s"] = round(used_c.value / dt / 1e6, 1)
    res["rx_device_over_host"] = round(res["rx_device_Mpackets_per_s"] / res["rx_host_Mpackets_per_s"], 1)
    ctx.close()
    if a.counts:
        with open(a.counts, "w") as f:
            json.dump(counts, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
