#!/usr/bin/env python3
"""The link emulator (include/ldpc_erasure_amd_link.h) on one GPU: the (2040,1530) code at S = 1024, 4096 frames of the reference's
datagram mix (the shape of tools/bench_wire_ragged.py), packed and sent by the fused sender: P = F n packets of 8 + S bytes; 10 %
Gilbert-Elliott loss at the cfg 3 parameters from ldpc_amd_synth_erasures_bursty, dup = 0.02 with flip, bad_sym = foreign = 0.005.

    plan W       ldpc_amd_fec_link_plan_dev at window W in {0, 128, 4096}: held against nothing -- its time and the compares it
                 stands for (every surviving packet sweeps the 2 (W + 1) packets around it, 4 compares each)
    apply        ldpc_amd_fec_link_apply_dev with the plan of W = 128: the row gather of Q packets
    apply_ragged ldpc_amd_fec_link_apply_ragged_dev with the same plan on the trimmed wire of the packets
    trim         Context.fec_trim_packets, re-measured here: what apply_ragged is held against, per byte moved
    copy         Context.copy_probe over the Q (8 + S) bytes apply moves: what apply is held against

The timed variants alternate step by step in ONE process, after a warm-up of each, device events around every step; median ms.
Before timing, the plan of W = 128 is checked against the numpy model (tools/link_model.py) on a prefix of the call, and apply and
apply_ragged against each other through land.

    python tools/bench_link.py [--frames 4096] [--steps 10] [--warmup 2] [--out profiles/link_bench.json]

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GE = (0.13, 0.8, 10.0)   # cfg 3: alpha, beta, good_transition_bias
WINDOWS = (0, 128, 4096)
LINK = dict(dup=0.02, bad_sym=0.005, foreign=0.005)
SEED, LOSS_SEED = 11, 12


def summary(v):
    return {"ms_per_step_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ldpc_erasure_codes_amd import api, codes
    import datagram_frames as dg
    import link_model as lm
    F, S = a.frames, a.S
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    L, hnd = ctx._L, ctx._h
    h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
    n, k, _ = ctx.code_info(h)
    N, P, plen = F * k, F * n, 8 + S
    gen = torch.Generator(device="cuda").manual_seed(5)
    ln = np.full(N, S - dg.PREFIX, dtype=np.int64)
    ln[::17] = dg.CONTEXT_BYTES
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    data = torch.randint(0, 256, (int(off[-1]),), dtype=torch.uint8, device="cuda", generator=gen)
    packets = torch.empty((P, plen), dtype=torch.uint8, device="cuda")
    ctx.fec_encode_packets_device(h, ctx.fec_pack_datagrams(data, off, k, S), 1, 0, out=packets)
    del data
    wire = api.Wire(torch.empty(P * plen, dtype=torch.uint8, device="cuda"), torch.empty(P + 1, dtype=torch.int64, device="cuda"))
    ctx.fec_trim_packets(packets, k, out=wire)
    lost = torch.empty(P, dtype=torch.uint8, device="cuda")
    ctx.synth_erasures_bursty(LOSS_SEED, 0, P, 1, *GE, lost)
    torch.cuda.synchronize()
    total = int(wire.offset[-1])
    survivors = P - int(lost.sum(dtype=torch.int64))

    cap = 2 * P
    src = torch.empty(cap, dtype=torch.int32, device="cuda")
    fate = torch.empty(cap, dtype=torch.int16, device="cuda")
    count = torch.empty(1, dtype=torch.int64, device="cuda")

    def params(W):
        return api.LinkParams(SEED, 0, W, api.LINK_DUP_FLIP, LINK["dup"], LINK["bad_sym"], LINK["foreign"])

    def plan(W):
        ctx._check(L.ldpc_amd_fec_link_plan_dev(hnd, C.byref(params(W)), P, lost.data_ptr(), src.data_ptr(), fate.data_ptr(), cap, count.data_ptr()),
                   "fec_link_plan_dev")

    # the plan the gathers run with, checked against the model on a prefix: a call of its first M packets has the same arrivals up
    # to the first entry of a packet the window lets the cut reach
    plan(128)
    torch.cuda.synchronize()
    Q = int(count[0])
    M = 20000
    m_src, m_fate = lm.plan(lm.Params(SEED, 0, 128, lm.DUP_FLIP, LINK["dup"], LINK["bad_sym"], LINK["foreign"]), M, lost[:M].cpu().numpy())
    safe = int(np.argmax(m_src >= M - 130))
    if not (safe > M // 2 and np.array_equal(src[:safe].cpu().numpy(), m_src[:safe]) and
            np.array_equal(fate[:safe].cpu().numpy().view(np.uint16), m_fate[:safe])):
        raise SystemExit("the plan differs from the model")
    out = torch.empty((cap, plen), dtype=torch.uint8, device="cuda")            # (cap rows: the host does not know Q)
    wire_out = api.Wire(torch.empty(2 * total, dtype=torch.uint8, device="cuda"), torch.empty(cap + 1, dtype=torch.int64, device="cuda"))

    def run_apply():
        ctx._check(L.ldpc_amd_fec_link_apply_dev(hnd, packets.data_ptr(), P, S, src.data_ptr(), fate.data_ptr(), count.data_ptr(), cap, out.data_ptr(),
                                                 None, None), "fec_link_apply_dev")

    def run_ragged():
        ctx._check(L.ldpc_amd_fec_link_apply_ragged_dev(hnd, wire.bytes.data_ptr(), total, wire.offset.data_ptr(), P, src.data_ptr(), fate.data_ptr(),
                                                        count.data_ptr(), cap, wire_out.bytes.data_ptr(), 2 * total, wire_out.offset.data_ptr(), None),
                   "fec_link_apply_ragged_dev")

    def run_trim():
        ctx.fec_trim_packets(packets, k, out=wire)

    # apply against apply_ragged through land, on the entries that are not flipped (the fixed-stride flip covers the zeros a short
    # datagram leaves behind it, land fills zeros in)
    run_apply()
    run_ragged()
    torch.cuda.synchronize()
    total_out = int(wire_out.offset[Q])
    landed, st = ctx.fec_land_packets(wire_out.bytes[:total_out], wire_out.offset[:Q + 1], S)
    plain = (fate[:Q] & api.LINK_FLIPPED) == 0
    if int(st.max()) != api.WIRE_LANDED or not torch.equal(landed[plain], out[:Q][plain]):
        raise SystemExit("apply_ragged + land differs from apply")
    del landed, st, plain

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(body):
        torch.cuda.synchronize()
        ev[0].record()
        body()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    # the gathers need the plan of W = 128 in src / fate: the plans are timed first, W = 128 last
    variants = [(f"plan_W{W}", (lambda W=W: plan(W))) for W in (0, 4096, 128)]
    ms = {}
    for group in (variants, [("apply", run_apply), ("apply_ragged", run_ragged), ("trim", run_trim)]):
        for _ in range(a.warmup):
            for _, fn in group:
                timed(fn)
        for nm, _ in group:
            ms[nm] = []
        for _ in range(a.steps):
            for nm, fn in group:
                ms[nm].append(timed(fn))
    med = {nm: statistics.median(v) for nm, v in ms.items()}
    info = ctx.fec_link_info()
    # the yardstick, in the same run: a streaming copy of the Q (8 + S) bytes apply moves
    moved = min(Q, P) * plen
    copy_ms = ctx.copy_probe(packets.view(-1), out.view(-1), reps=a.steps, nbytes=moved)
    per_byte = {"apply_ragged": med["apply_ragged"] * 1e9 / (2 * total_out), "trim": med["trim"] * 1e9 / (2 * total)}
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "packets": P, "survivors": survivors, "arrivals": Q,
           "loss": {"model": "Gilbert-Elliott", "alpha_beta_bias": list(GE), "fraction": round(1 - survivors / P, 4)}, "link": LINK,
           "steps": a.steps, "warmup": a.warmup, "link_info": info,
           "variants": {nm: summary(v) for nm, v in ms.items()},
           # every surviving packet sweeps the 2 (W + 1) packets around it, its two keys against their two: 4 compares each
           "plan_compares": {f"W{W}": survivors * 2 * (W + 1) * 4 for W in WINDOWS},
           "plan_compares_per_ns": {f"W{W}": round(survivors * 2 * (W + 1) * 4 / (med[f"plan_W{W}"] * 1e6), 1) for W in WINDOWS},
           "apply_bytes_read_plus_written": 2 * moved, "wire_bytes_in": total, "wire_bytes_out": total_out,
           "copy_probe": {"bytes": moved, "ms_best": round(copy_ms, 4), "TBps_read_plus_write": round(2 * moved / (copy_ms * 1e-3) / 1e12, 3)},
           "apply_over_copy": round(med["apply"] / copy_ms, 3),
           "apply_TBps_read_plus_write": round(2 * moved / (med["apply"] * 1e-3) / 1e12, 3),
           "apply_ragged_TBps_read_plus_write": round(2 * total_out / (med["apply_ragged"] * 1e-3) / 1e12, 3),
           "picoseconds_per_byte_moved": {nm: round(v, 4) for nm, v in per_byte.items()},
           "apply_ragged_over_trim": round(per_byte["apply_ragged"] / per_byte["trim"], 3)}
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
