#!/usr/bin/env python3
"""Interleaving depth on the multi-flow wire (include/ldpc_erasure_amd_interleave_flows.h) on one GPU, BASELINE shape: the
(2040,1530) code at S = 1024, 4096 frames split evenly over the flows.

    quality   blocks decoded (status <= 1) of the 4096 sent, over 4 / 8 / 64 flows at depth 1 / 4 / 8: FecTxFlows(depth, round
              robin) -> FecLink (no reordering, the Gilbert-Elliott loss of BASELINE cfg 3 by wire position) ->
              FecRxWindowFlows(W = 16, A = 10, depth).decode_mixed + decode_flush_many.  Says at which flow count depth still
              pays over round-robin multiplexing alone.
    receiver  FecRxWindowFlows(W = 16, A = 10, depth = 8).decode_mixed on the depth-8 round-robin wire against depth 1 on the
              depth-1 wire, 10 % uniform loss on both, over 1 / 8 / 64 flows, the two alternating step by step in one process,
              every step on a fresh object, device events around the call
    sender    Context.fec_encode_packets_flows_interleaved_device (depth 8, round robin) against
              Context.fec_encode_packets_flows_device (round robin) over 8 / 64 / 256 flows, alternating likewise

    python tools/bench_flows_depth.py [--frames 4096] [--steps 10] [--warmup 2] [--out profiles/flows_depth_bench.json]

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GE_PARAMS = (0.13, 0.8, 10.0)   # bench.py's cfg 3 channel: alpha, beta, good_transition_bias
W, A = 16, 10
QUALITY_FLOWS, QUALITY_DEPTHS = (4, 8, 64), (1, 4, 8)
RECEIVER_FLOWS, SENDER_FLOWS, TIMED_DEPTH = (1, 8, 64), (8, 64, 256), 8


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
    import numpy as np
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
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "steps": a.steps, "window": W, "ahead_limit": A,
           "knobs": ctx.knobs()}

    def begin(nf):
        assert F % (nf * TIMED_DEPTH) == 0, "whole groups per flow"
        return np.arange(nf + 1, dtype=np.int64) * (F // nf)

    def send(nf, D):
        """The round-robin wire of nf flows at depth D: (packets, flow_of)."""
        pk, flow_of, _ = ctx.fec_tx_flows(h, S, nf, depth=D).send(src, begin(nf), api.TX_ROUND_ROBIN, out=out)
        return pk, flow_of

    def timed(variants):
        ms = {name: [] for name, _ in variants}
        last = {}
        for i in range(a.warmup + a.steps):
            for name, fn in variants:
                torch.cuda.synchronize()
                ev[0].record()
                last[name] = fn()
                ev[1].record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms[name].append(ev[0].elapsed_time(ev[1]))
        return ms, last

    # ---- quality: the cfg 3 Gilbert-Elliott loss by wire position, no reordering
    lost = torch.empty(F * n, dtype=torch.uint8, device="cuda")
    ctx.synth_erasures_bursty(79, 0, F * n, 1, *GE_PARAMS, lost)
    res["quality"] = {"channel": {"alpha": GE_PARAMS[0], "beta": GE_PARAMS[1], "good_transition_bias": GE_PARAMS[2], "seed": 79},
                      "lost_fraction": round(float(lost.float().mean().item()), 5)}
    for nf in QUALITY_FLOWS:
        per = F // nf
        for D in QUALITY_DEPTHS:
            pk, flow_of = send(nf, D)
            arrived, fo, _, _ = ctx.fec_link(seed=5, window=0).send(pk, lost, flow_of)
            with ctx.fec_rx_window_flows(nf, n, k, S, W, A, depth=D) as rx:
                closes, blocks, fr, consumed, offered = rx.decode_mixed(h, arrived, fo, per + W)
                assert np.array_equal(consumed, offered)
                ok = int((fr.status.cpu().numpy() <= 1).sum()) if len(blocks) else 0
                closed = len(blocks)
                del fr
                closes, blocks, fr = rx.decode_flush_many(h)
                ok += int((fr.status.cpu().numpy() <= 1).sum()) if len(blocks) else 0
                closed += len(blocks)
                tot = [rx.stats(f) for f in range(nf)]
                res["quality"]["flows_%d_depth_%d" % (nf, D)] = {
                    "blocks_decoded": ok, "blocks_handed_out": closed, "blocks_sent": F,
                    "totals": {key: int(sum(t[key] for t in tot)) for key in tot[0]}}
            del arrived, fo, fr
            torch.cuda.empty_cache()

    # ---- receiver: decode_mixed at depth 8 against depth 1, the same uniform loss pattern on both wires
    keep = torch.rand(F * n, device="cuda", generator=g) >= a.loss
    res["receiver"] = {}
    for nf in RECEIVER_FLOWS:
        per = F // nf
        wires = {}
        for name, D in (("depth_1", 1), ("depth_%d" % TIMED_DEPTH, TIMED_DEPTH)):
            pk, flow_of = send(nf, D)
            torch.cuda.synchronize()
            wires[name] = (pk[keep].contiguous(), flow_of[keep].contiguous(), D)
        got = {}

        def step(name):
            pk, fo, D = wires[name]
            rx = ctx.fec_rx_window_flows(nf, n, k, S, W, A, depth=D)
            torch.cuda.synchronize()
            ev[0].record()
            closes, blocks, fr, consumed, offered = rx.decode_mixed(h, pk, fo, per)
            ev[1].record()
            torch.cuda.synchronize()
            got[name] = {"blocks_closed": int(len(blocks)), "packets_consumed": int(consumed.sum()),
                         "frames_decoded": int((fr.status.cpu().numpy() <= 1).sum()), "path": ctx.fec_rx_window_flows_info()["path"]}
            rx.close()
            return ev[0].elapsed_time(ev[1])

        ms = {name: [] for name in wires}
        for i in range(a.warmup + a.steps):
            for name in wires:
                t = step(name)
                if i >= a.warmup:
                    ms[name].append(t)
        packets = int(wires["depth_1"][0].shape[0])
        r = {name: dict(stats(v), packets=packets, **got[name]) for name, v in ms.items()}
        d = statistics.median(ms["depth_%d" % TIMED_DEPTH]) - statistics.median(ms["depth_1"])
        r["depth_%d_over_depth_1" % TIMED_DEPTH] = round(statistics.median(ms["depth_%d" % TIMED_DEPTH]) / statistics.median(ms["depth_1"]), 4)
        r["difference_ns_per_packet_of_a_flow"] = round(d * 1e6 / (packets / nf), 3)   # the flows' scans run side by side
        res["receiver"]["flows_%d" % nf] = r
        del wires
        torch.cuda.empty_cache()

    # ---- sender: the flows-interleaved call against the flows call, round robin
    res["sender"] = {}
    for nf in SENDER_FLOWS:
        fb = begin(nf)
        variants = [("flows", lambda: ctx.fec_encode_packets_flows_device(h, src, fb, 1, 0, api.TX_ROUND_ROBIN, out=out, want_flow_of=False)),
                    ("flows_depth_%d" % TIMED_DEPTH,
                     lambda: ctx.fec_encode_packets_flows_interleaved_device(h, src, fb, 1, 0, api.TX_ROUND_ROBIN, TIMED_DEPTH, out=out,
                                                                             want_flow_of=False))]
        ms, _ = timed(variants)
        r = {name: stats(v) for name, v in ms.items()}
        r["paths"] = [ctx.fec_sender_flows_info()["path"], ctx.fec_sender_flows_ilv_info()["path"]]
        r["depth_%d_over_flows" % TIMED_DEPTH] = round(statistics.median(ms["flows_depth_%d" % TIMED_DEPTH]) / statistics.median(ms["flows"]), 4)
        res["sender"]["flows_%d" % nf] = r
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
