#!/usr/bin/env python3
"""Where the windowed receiver's time goes at depth 1 and at depth 8 (include/ldpc_erasure_amd_interleave.h): the workload for a
kernel trace, and the summary of two traces -- the source of profiles/interleave_rx_kernel_stats.csv.

    rocprofv3 --kernel-trace --stats -d prof_out/depth1 -- python tools/trace_interleave_rx.py run 1
    rocprofv3 --kernel-trace --stats -d prof_out/depth8 -- python tools/trace_interleave_rx.py run 8
    python tools/trace_interleave_rx.py summarize prof_out/depth1 prof_out/depth8 --out profiles/interleave_rx_kernel_stats.csv

run D: the (2040,1530) code at S = 1024, 4096 frames through the depth-D sender, 10 % uniform loss, then three
FecRxWindow(W = 16, A = 10, depth = D).decode_many calls, each on a fresh object (tools/bench_interleave.py's receiver leg).
summarize: per run and kernel of the library (the framework's own kernels are left out) calls, total, mean, min and max ms, from
the databases the profiler wrote under the two folders."""
import argparse
import csv
import glob
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAGS = ("depth_1_on_straight_wire", "depth_8_on_depth_8_wire")


def run(D, frames, S, steps):
    import torch
    from ldpc_erasure_codes_amd import api, codes
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
    n, k, _ = ctx.code_info(h)
    g = torch.Generator(device="cuda").manual_seed(11)
    src = torch.randint(0, 256, (frames, k, S), dtype=torch.uint8, device="cuda", generator=g)
    out = ctx.fec_encode_packets_interleaved_device(h, src, D, 1, 0)
    keep = torch.rand(frames * n, device="cuda", generator=g) >= 0.10
    pk = out[keep].contiguous()
    del out, src
    for _ in range(steps):
        rx = ctx.fec_rx_window(n, k, S, 16, 10, depth=D)
        b, fr, used = rx.decode_many(h, pk, frames)
        torch.cuda.synchronize()
        rx.close()
    print("blocks", len(b), "packets", int(used))
    ctx.close()


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name).replace("void ", "").replace("ldpc_amd::", "")
    m = re.match(r"[A-Za-z_0-9:]+", name)
    return m.group(0) if m else name[:40]


def summarize(folders, out):
    rows = []
    for folder, tag in zip(folders, TAGS):
        db = glob.glob(os.path.join(folder, "**", "*.db"), recursive=True)[0]
        acc = {}
        for name, start, end in sqlite3.connect(db).execute("select name, start, end from kernels"):
            if "at::native" in name or "rocprim" in name or "rocclr" in name:
                continue
            acc.setdefault(short(name), []).append(end - start)
        for kern, v in sorted(acc.items(), key=lambda kv: -sum(kv[1])):
            rows.append([tag, kern, len(v), round(sum(v) / 1e6, 4), round(sum(v) / len(v) / 1e6, 4), round(min(v) / 1e6, 4), round(max(v) / 1e6, 4)])
    with open(out, "w") as f:
        w = csv.writer(f)
        w.writerow(["run", "kernel", "calls", "total_ms", "mean_ms", "min_ms", "max_ms"])
        w.writerows(rows)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("depth", type=int)
    r.add_argument("--frames", type=int, default=4096)
    r.add_argument("--S", type=int, default=1024)
    r.add_argument("--steps", type=int, default=3)
    s = sub.add_parser("summarize")
    s.add_argument("folders", nargs=2)
    s.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.cmd == "run":
        run(a.depth, a.frames, a.S, a.steps)
    else:
        summarize(a.folders, a.out)


if __name__ == "__main__":
    main()
