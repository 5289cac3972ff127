#!/usr/bin/env python3
"""The close rule of the windowed receiver as a value (include/ldpc_erasure_amd_rx_rule.h) on one GPU: the default rule beside the
rule of fec_rx_rule_mds, on the streams of tools/bench_rs_wire.py -- RS(255,192) beside the (2040,1530) LDPC code, both over
4096 * 2040 = 32768 * 255 wire packets.

    quality   tools/bench_rs_wire.py's quality part under both rules: one Gilbert-Elliott loss trace by wire position (BASELINE cfg 3,
              seed 79), no reordering, flush at the end, S = 64, A = 10: LDPC at depth 1 and 8 (W = 16), RS at depth 1, 8 (W = 16) and
              16 (W = 32).  Per run: source symbols delivered of those sent, blocks decoded, blocks handed out, the receiver's totals.
              RS runs also count the blocks of which k or more packets ARRIVED -- what the channel alone leaves decodable -- and how
              many of THOSE the receiver delivered.  The LDPC code is not MDS: its runs under the MDS preset are reported as found.
    timing    decode_many (LDPC, depth 8) and rs_decode_many (RS, depth 8) on a fresh object over a wire at 10 % uniform loss, S = 1024,
              W = 16, A = 10, under both rules, alternating in one process.  The default rule is timed twice (default_a, default_b): the
              spread of its two medians is the noise the ruled kernel's time is to be read against.  The ruled scan's time is reported,
              not bounded.

    python tools/bench_rx_rule.py [--blocks 32768] [--rx-blocks 4096] [--steps 5] [--warmup 1] [--out profiles/rx_rule_bench.json]

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

GE_PARAMS = (0.13, 0.8, 10.0)   # bench.py's cfg 3 channel: alpha, beta, good_transition_bias
RS_N, RS_K = 255, 192
A = 10


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=32768, help="RS blocks; a multiple of 16 (the LDPC runs take blocks / 8 frames)")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--rx-blocks", type=int, default=4096)
    ap.add_argument("--loss", type=float, default=0.10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from ldpc_erasure_codes_amd import api, codes
    B, S, n, k = a.blocks, a.S, RS_N, RS_K
    F = B // 8
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    rs = ctx.rs_create(n, k)
    h = ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
    ln, lk, _ = ctx.code_info(h)
    assert F * ln == B * n
    g = torch.Generator(device="cuda").manual_seed(11)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"device": torch.cuda.get_device_name(0), "rs": [n, k], "ldpc": [ln, lk], "blocks": B, "steps": a.steps, "ahead_limit": A}

    def rules(nn, kk, depth):
        return {"default": None, "mds": api.fec_rx_rule_mds(nn, kk, depth)}

    # ---- quality
    QS = 64
    P = B * n
    lost = torch.empty(P, dtype=torch.uint8, device="cuda")
    ctx.synth_erasures_bursty(79, 0, P, 1, *GE_PARAMS, lost)
    res["quality"] = {"channel": {"alpha": GE_PARAMS[0], "beta": GE_PARAMS[1], "good_transition_bias": GE_PARAMS[2], "seed": 79}, "S": QS,
                      "lost_fraction": round(float(lost.float().mean().item()), 5)}
    rsrc = torch.randint(0, 256, (B, k, QS), dtype=torch.uint8, device="cuda", generator=g)
    lsrc = torch.randint(0, 256, (F, lk, QS), dtype=torch.uint8, device="cuda", generator=g)

    def run(name, kind, depth, W):
        if kind == "rs":
            wire = ctx.fec_rs_encode_packets_device(rs, rsrc, depth, block0=0)
            nn, kk, sent = n, k, B
            # what the channel alone leaves: block i of group g owns the wire positions (g n + j) depth + i (block0 = 0, whole groups)
            kept = (lost == 0).view(B // depth, n, depth).sum(1).reshape(-1)   # by block serial
            decodable = kept >= kk
        else:
            wire = ctx.fec_encode_packets_interleaved_device(h, lsrc, depth, 1, 0)
            nn, kk, sent = ln, lk, F
        arrived = ctx.fec_link(seed=5, window=0).send(wire, lost=lost)[0]
        del wire
        out = {"depth": depth, "window": W, "span_packets": depth * nn, "blocks_sent": sent, "source_symbols_sent": sent * kk}
        if kind == "rs":
            out["blocks_with_k_arrived"] = int(decodable.sum().item())
        for rname, rule in rules(nn, kk, depth).items():
            delivered = decoded = handed = flushed = 0
            with ctx.fec_rx_window(nn, kk, QS, W, A, depth=depth, rule=rule) as rx:
                def take(b, r):
                    nonlocal delivered, decoded, handed
                    if not len(b):
                        return
                    handed += len(b)
                    if kind == "rs":
                        ok = (r[2] == 0)
                        decoded += int(ok.sum().item())
                        delivered += int(ok.sum().item()) * kk
                    else:
                        decoded += int((r.status <= 1).sum().item())
                        delivered += int((kk - r.residual_src).sum().item())
                pos = 0
                while pos < arrived.shape[0]:
                    if kind == "rs":
                        b, msg, received, status, used = rx.rs_decode_many(rs, arrived[pos:], 2048)
                        take(b, (msg, received, status))
                    else:
                        b, fr, used = rx.decode_many(h, arrived[pos:], 256)
                        take(b, fr)
                    pos += used
                if kind == "rs":
                    b, msg, received, status = rx.rs_decode_flush(rs)
                    take(b, (msg, received, status))
                else:
                    b, fr = rx.decode_flush(h)
                    take(b, fr)
                flushed = len(b)
                t = rx.stats()
                used_rule = rx.rule
            q = {"rule": list(used_rule), "blocks_handed_out": handed, "blocks_decoded": decoded, "source_symbols_delivered": delivered,
                 "delivered_fraction": round(delivered / (sent * kk), 6), "flushed": flushed,
                 "forced_closes_at_most": t["ahead_total"] // (A + 1) + flushed, "totals": t}
            if kind == "rs":
                # a decoded RS block had k symbols, and only a block of which k packets arrived can have them
                q["decodable_blocks_delivered"] = decoded
                q["of_the_channels_decodable"] = round(decoded / max(1, out["blocks_with_k_arrived"]), 6)
            out[rname] = q
        res["quality"][name] = out
        del arrived
        torch.cuda.empty_cache()

    run("ldpc_depth_1", "ldpc", 1, 16)
    run("ldpc_depth_8", "ldpc", 8, 16)
    run("rs_depth_1", "rs", 1, 16)
    run("rs_depth_8", "rs", 8, 16)
    run("rs_depth_16", "rs", 16, 32)
    del rsrc, lsrc, lost
    torch.cuda.empty_cache()

    # ---- timing
    D, W = 8, 16
    RB = min(a.rx_blocks, B)
    RF = RB // 8

    def timed(variants, steps, warmup):
        ms = {name: [] for name, _ in variants}
        for i in range(warmup + steps):
            for name, fn in variants:
                torch.cuda.synchronize()
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                if i >= warmup:
                    ms[name].append(ev[0].elapsed_time(ev[1]))
        return ms

    res["timing"] = {"S": S, "depth": D, "window": W, "loss": a.loss, "note": "whole calls on a fresh object, creation and the host's read-backs included"}
    for kind in ("rs", "ldpc"):
        if kind == "rs":
            src = torch.randint(0, 256, (RB, k, S), dtype=torch.uint8, device="cuda", generator=g)
            wire = ctx.fec_rs_encode_packets_device(rs, src, D, block0=0)
            nn, kk, cap = n, k, RB
        else:
            src = torch.randint(0, 256, (RF, lk, S), dtype=torch.uint8, device="cuda", generator=g)
            wire = ctx.fec_encode_packets_interleaved_device(h, src, D, 1, 0)
            nn, kk, cap = ln, lk, RF
        keep = torch.rand(wire.shape[0], device="cuda", generator=g) >= a.loss
        pk = wire[keep].contiguous()
        del wire, src, keep
        got = {}

        def call(name, rule):
            def fn():
                with ctx.fec_rx_window(nn, kk, S, W, A, depth=D, rule=rule) as rx:
                    if kind == "rs":
                        b, msg, received, status, used = rx.rs_decode_many(rs, pk, cap)
                        ok = int((status == 0).sum().item())
                    else:
                        b, fr, used = rx.decode_many(h, pk, cap)
                        ok = int((fr.status <= 1).sum().item())
                    got[name] = {"blocks": int(len(b)), "consumed": int(used), "decoded": ok, "totals": rx.stats()}
                    torch.cuda.synchronize()
            return fn

        r = rules(nn, kk, D)
        ms = timed([("default_a", call("default_a", r["default"])), ("mds", call("mds", r["mds"])), ("default_b", call("default_b", r["default"]))],
                   a.steps, a.warmup)
        med = {name: statistics.median(v) for name, v in ms.items()}
        t = {name: dict(stats(v), **got[name]) for name, v in ms.items()}
        t.update(call="rs_decode_many" if kind == "rs" else "decode_many", blocks_sent=cap, packets=int(pk.shape[0]), rule_mds=list(r["mds"]),
                 default_spread_ms=round(abs(med["default_a"] - med["default_b"]), 4),
                 mds_over_default=round(med["mds"] / min(med["default_a"], med["default_b"]), 4))
        res["timing"][kind] = t
        del pk
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
