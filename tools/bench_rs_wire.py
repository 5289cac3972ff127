#!/usr/bin/env python3
"""Reed-Solomon on the FEC wire (include/ldpc_erasure_amd_rs_wire.h) on one GPU: RS(255,192) beside the (2040,1530) LDPC code, both
over 4096 * 2040 = 32768 * 255 wire packets.

    sender    Context.fec_rs_encode_packets_device (fused) at depth 8, S = 1024, 32768 blocks, against the composition the library
              offered before it: Context.rs_encode + Context.fec_packetize_device + one index_select by the layout.  The composition
              is timed twice in the alternation (composed_a, composed_b): the spread of its two medians is the margin the fused call
              has to beat.  For context: the LDPC interleaved sender at depth 1 on 4096 frames, and rs_encode alone.
    receiver  FecRxWindow(16, 10, depth = 8).rs_decode_many on a fresh object at 10 % uniform loss, beside the same object's push_many
              followed by Context.rs_decode_frames.
    quality   one Gilbert-Elliott loss trace by wire position (BASELINE cfg 3), no reordering, flush at the end, S = 64 (what is
              delivered does not depend on S): LDPC at depth 1 and 8 (W = 16), RS at depth 1, 8 (W = 16) and 16 (W = 32), A = 10.
              Per run: source symbols delivered of those sent, blocks decoded, blocks handed out, the receiver's totals, and two
              bounds on the forced closes -- at least the blocks handed out at or below the rule's lower threshold (RS: from
              `received`), at most ahead_total / (A + 1) plus the blocks of the flush.  RS runs also count the blocks of which k or
              more packets ARRIVED: what the channel alone leaves decodable, whatever the receiver then does with them.

    python tools/bench_rs_wire.py [--blocks 32768] [--steps 5] [--warmup 1] [--out profiles/rs_wire_bench.json]

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
    ap.add_argument("--blocks", type=int, default=32768, help="RS blocks; a multiple of 8 (the LDPC runs take blocks / 8 frames)")
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--rx-blocks", type=int, default=4096)
    ap.add_argument("--loss", type=float, default=0.10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    import interleave_model as im
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
    res = {"device": torch.cuda.get_device_name(0), "rs": [n, k], "ldpc": [ln, lk], "S": S, "blocks": B, "steps": a.steps}

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

    # ---- sender
    D = 8
    src = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty((B * n, 8 + S), dtype=torch.uint8, device="cuda")
    cw = torch.empty((B, n, S), dtype=torch.uint8, device="cuda")
    straight = torch.empty((B * n, 8 + S), dtype=torch.uint8, device="cuda")
    placed = torch.empty((B * n, 8 + S), dtype=torch.uint8, device="cuda")
    frame, row = im.order(B, n, 0, D)
    index = torch.from_numpy(frame * n + row).cuda()

    def fused():
        ctx.fec_rs_encode_packets_device(rs, src, D, block0=0, out=out)

    def composed():
        ctx.rs_encode(rs, n, k, src, out=cw)
        ctx.fec_packetize_device(cw, api.FEC_CLASS_RS, 0, out=straight)
        torch.index_select(straight, 0, index, out=placed)

    ms = timed([("composed_a", composed), ("fused", fused), ("composed_b", composed), ("rs_encode_alone", lambda: ctx.rs_encode(rs, n, k, src, out=cw))],
               a.steps, a.warmup)
    same = bool(torch.equal(out, placed))
    del cw, straight, placed, index
    torch.cuda.empty_cache()
    lsrc = src.view(-1)[:F * lk * S].view(F, lk, S)   # (any bytes do for the context line)
    ms.update(timed([("ldpc_interleaved_depth_1", lambda: ctx.fec_encode_packets_interleaved_device(h, lsrc, 1, 1, 0, out=out))], a.steps, a.warmup))
    med = {name: statistics.median(v) for name, v in ms.items()}
    res["sender"] = {name: stats(v) for name, v in ms.items()}
    res["sender"].update(path=ctx.fec_rs_sender_info()["path"], depth=D, same_bytes=same,
                         margin_ms=round(abs(med["composed_a"] - med["composed_b"]), 4),
                         fused_over_composed=round(med["fused"] / min(med["composed_a"], med["composed_b"]), 4),
                         fused_below_composed_by_more_than_the_margin=bool(min(med["composed_a"], med["composed_b"]) - med["fused"] >
                                                                           abs(med["composed_a"] - med["composed_b"])))

    # ---- receiver
    RB = min(a.rx_blocks, B)
    ctx.fec_rs_encode_packets_device(rs, src[:RB], D, block0=0, out=out[:RB * n])
    torch.cuda.synchronize()
    keep = torch.rand(RB * n, device="cuda", generator=g) >= a.loss
    pk = out[:RB * n][keep].contiguous()
    got = {}

    def one_call():
        with ctx.fec_rx_window(n, k, S, 16, A, depth=D) as rx:
            b, msg, received, status, used = rx.rs_decode_many(rs, pk, RB)
            got["rs_decode_many"] = {"blocks": int(len(b)), "consumed": int(used), "decoded": int((status == 0).sum().item())}
            torch.cuda.synchronize()

    def two_calls():
        with ctx.fec_rx_window(n, k, S, 16, A, depth=D) as rx:
            b, sym, er, used = rx.push_many(pk, RB)
            r = ctx.rs_decode_frames(rs, sym, er)
            got["push_many_then_rs_decode_frames"] = {"blocks": int(len(b)), "consumed": int(used), "decoded": int((r.status == 0).sum().item())}
            torch.cuda.synchronize()

    ms = timed([("push_many_then_rs_decode_frames", two_calls), ("rs_decode_many", one_call), ("push_many_then_rs_decode_frames_again", two_calls)],
               a.steps, a.warmup)
    res["receiver"] = {name: dict(stats(v), **got.get(name, {})) for name, v in ms.items()}
    res["receiver"].update(blocks_sent=RB, packets=int(pk.shape[0]), loss=a.loss, info=ctx.fec_rs_receiver_info(),
                           note="whole calls, object creation and the host's read-backs included")
    del pk, keep, src, lsrc, out
    torch.cuda.empty_cache()

    # ---- quality
    QS = 64
    P = B * n
    lost = torch.empty(P, dtype=torch.uint8, device="cuda")
    ctx.synth_erasures_bursty(79, 0, P, 1, *GE_PARAMS, lost)
    res["quality"] = {"channel": {"alpha": GE_PARAMS[0], "beta": GE_PARAMS[1], "good_transition_bias": GE_PARAMS[2], "seed": 79}, "S": QS,
                      "ahead_limit": A, "lost_fraction": round(float(lost.float().mean().item()), 5)}
    rsrc = torch.randint(0, 256, (B, k, QS), dtype=torch.uint8, device="cuda", generator=g)
    lsrc = torch.randint(0, 256, (F, lk, QS), dtype=torch.uint8, device="cuda", generator=g)
    km_rs = k + int(np.floor((n - k) * 0.2 + 0.5))

    def run(name, kind, depth, W):
        if kind == "rs":
            wire = ctx.fec_rs_encode_packets_device(rs, rsrc, depth, block0=0)
            nn, kk, sent = n, k, B
        else:
            wire = ctx.fec_encode_packets_interleaved_device(h, lsrc, depth, 1, 0)
            nn, kk, sent = ln, lk, F
        arrived = ctx.fec_link(seed=5, window=0).send(wire, lost=lost)[0]
        delivered = decoded = handed = low = flushed = 0
        with ctx.fec_rx_window(nn, kk, QS, W, A, depth=depth) as rx:
            def take(b, r):
                nonlocal delivered, decoded, handed, low
                if not len(b):
                    return
                handed += len(b)
                if kind == "rs":
                    ok = (r[2] == 0)
                    decoded += int(ok.sum().item())
                    delivered += int(ok.sum().item()) * kk
                    low += int((r[1] <= km_rs).sum().item())
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
        q = {"depth": depth, "window": W, "span_packets": depth * nn, "blocks_sent": sent, "blocks_handed_out": handed, "blocks_decoded": decoded,
             "source_symbols_sent": sent * kk, "source_symbols_delivered": delivered, "delivered_fraction": round(delivered / (sent * kk), 6),
             "flushed": flushed, "forced_closes_at_most": t["ahead_total"] // (A + 1) + flushed, "totals": t}
        if kind == "rs":
            q["forced_closes_at_least"] = low
            # what the channel alone leaves: block i of group g owns the wire positions (g n + j) depth + i (block0 = 0, whole groups)
            kept = (lost == 0).view(B // depth, n, depth).sum(1)
            q["blocks_with_k_arrived"] = int((kept >= kk).sum().item())
        res["quality"][name] = q
        del wire, arrived
        torch.cuda.empty_cache()

    run("ldpc_depth_1", "ldpc", 1, 16)
    run("ldpc_depth_8", "ldpc", 8, 16)
    run("rs_depth_1", "rs", 1, 16)
    run("rs_depth_8", "rs", 8, 16)
    run("rs_depth_16", "rs", 16, 32)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
