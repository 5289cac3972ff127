#!/usr/bin/env python3
"""Device time of the S = 1 decoder on a staircase code (tools/relax_model.py): the time-stamp relaxation (PEEL_RELAX = 1, the
default) against the serial per-solve loop (PEEL_RELAX = 0), PEEL kind of the library's own profiling brackets.

The relaxation settles one check of a chunk per round on a chain, about m * m / 64 evaluations against m serial solves
(DESIGN.md section 4.1b); this prints what that costs, one JSON line per erasure pattern, so that a later change can decide
whether plan_relax's `keys_fit` (kernels.hip) should look at the code's chain depth.

    python tools/time_relax_chain.py [--m 1024] [--frames 4096] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import relax_model as rm  # noqa: E402

from ldpc_erasure_codes_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m, F = a.m, a.frames
    code = rm.staircase(np.random.default_rng(m), m, m, 4)
    tab = rm.Tables(code)
    lines = []
    with api.Context(0) as ctx:
        h = ctx.register_code(code)
        cw = ctx.encode(h, synth.source(1, 0, F, code.k, 1)[:, :, 0])
        patterns = {"all_parity": np.zeros((F, code.n), dtype=np.uint8), "uniform_10_percent": synth.erasures_uniform(2, 0, F, code.n, 0.10)}
        patterns["all_parity"][:, code.k:] = 1
        for pname, era in patterns.items():
            sym = cw.copy()
            sym[era.astype(bool)] = 0
            line = {"code": "staircase", "m": m, "n": code.n, "frames": F, "S": 1, "pattern": pname, "max_sweeps": 10,
                    "model_evaluations_frame0": rm.relax(tab, era[0], 10)["evaluations"], "model_budget": rm.eval_budget(tab.nch, m, 10)}
            outs = {}
            for relax in ("1", "0"):
                ctx.configure("PEEL_RELAX", relax)
                outs[relax] = ctx.decode(h, sym, era)        # warm-up, and the bytes for the comparison below
                ctx.set_profiling(1)
                ctx.get_profile()
                times = []
                for _ in range(a.reps):
                    ctx.decode(h, sym, era)
                    ms, launches = ctx.get_profile()["peel"]
                    times.append(ms)
                ctx.set_profiling(0)
                key = "relax" if relax == "1" else "serial"
                line[key + "_kernel"] = ctx.profile_kernel_names()["peel"]
                line[key + "_peel_ms"] = [round(t, 4) for t in times]
                line[key + "_peel_ms_median"] = round(float(np.median(times)), 4)
                line[key + "_launches"] = int(launches)
            ctx.configure("PEEL_RELAX", None)
            line["identical"] = all(np.array_equal(x, y) for x, y in zip(outs["1"], outs["0"]))
            line["decoded"] = bool(np.array_equal(outs["1"][0][outs["1"][3] == 0], cw[outs["1"][3] == 0]))
            line["relax_over_serial"] = round(line["relax_peel_ms_median"] / max(line["serial_peel_ms_median"], 1e-9), 2)
            lines.append(line)
            print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    return 0 if all(ln["identical"] and ln["decoded"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
