#!/usr/bin/env python3
"""The Reed-Solomon decoder on rows in place (include/ldpc_erasure_amd_rs_rows.h) on one GPU; S = 1024, 4096 blocks, 10 % uniform loss.

    decoder   Context.rs_decode_rows on packet words against Context.rs_decode_frames on the same blocks gathered beforehand (the
              gather is not timed), for RS(255,192) and RS(255,223).  rs_decode_frames is timed on both sides of the new call in
              the alternation: the distance of its two medians is the margin.  The gather alone is the third figure.
    receiver  a fresh FecRxWindow(16, 10, depth = 8) per step, RS(255,192): rs_decode_many fused, rs_decode_many with RX_PKT = 0
              (composed), and push_many followed by rs_decode_frames (timed on both sides); whole calls, object creation and the
              host's read-backs included -- the figures of DESIGN.md 4.4b.
    sender    with --parent-lib: Context.fec_rs_encode_packets_device (RS(255,192), 32768 blocks, depth 8) of this build against
              another build of the library, one child process per library and round, three alternating rounds (tools/ab_interleave.py's
              scheme); the bound is the other build's own spread between its rounds.

    python tools/bench_rs_rows.py [--blocks 4096] [--steps 5] [--warmup 1] [--parent-lib old.so] [--out profiles/rs_rows_bench.json]

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CODES = [(255, 192), (255, 223)]
W, A, D = 16, 10, 8


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def sender_child(so, blocks, S, steps, warmup):
    import torch
    from ldpc_erasure_codes_amd import api
    api.LIB_PATH = so
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n, k = CODES[0]
    rs = ctx.rs_create(n, k)
    src = torch.randint(0, 256, (blocks, k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
    out = torch.empty((blocks * n, 8 + S), dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        ev[0].record()
        ctx.fec_rs_encode_packets_device(rs, src, D, block0=0, out=out)
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    assert ctx.fec_rs_sender_info()["path"] == "fused"
    ctx.close()
    print(json.dumps({"rs_encode_packets_ms": statistics.median(ms)}))


def sender_ab(old, new, rounds, blocks, S, steps, warmup):
    acc = {old: [], new: []}
    for _ in range(rounds):
        for so in (old, new):
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--sender-child", os.path.abspath(so), "--sender-blocks", str(blocks),
                                "--S", str(S), "--steps", str(steps), "--warmup", str(warmup)], capture_output=True, text=True, timeout=600)
            if o.returncode:
                print(o.stderr[-2000:])
                sys.exit(1)
            acc[so].append(json.loads(o.stdout.strip().splitlines()[-1])["rs_encode_packets_ms"])
    res = {tag: {"per_round_ms": [round(x, 4) for x in acc[so]], "median_ms": round(statistics.median(acc[so]), 4),
                 "spread_ms": round(max(acc[so]) - min(acc[so]), 4)} for tag, so in (("parent", old), ("this", new))}
    diff = res["this"]["median_ms"] - res["parent"]["median_ms"]
    res.update(rounds=rounds, blocks=blocks, depth=D, this_minus_parent_ms=round(diff, 4),
               within_the_parents_spread=bool(abs(diff) <= res["parent"]["spread_ms"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--loss", type=float, default=0.10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sender-blocks", type=int, default=32768)
    ap.add_argument("--sender-child", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.sender_child:
        sender_child(a.sender_child, a.sender_blocks, a.S, a.steps, a.warmup)
        return
    import torch
    from ldpc_erasure_codes_amd import api
    B, S = a.blocks, a.S
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(11)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"device": torch.cuda.get_device_name(0), "S": S, "blocks": B, "loss": a.loss, "steps": a.steps, "decoder": {}}

    def timed(variants):
        ms = {name: [] for name, _ in variants}
        for i in range(a.warmup + a.steps):
            for name, fn in variants:
                torch.cuda.synchronize()
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ms[name].append(ev[0].elapsed_time(ev[1]))
        return ms

    def verdict(ms, new, old_a, old_b):
        med = {name: statistics.median(v) for name, v in ms.items()}
        margin = abs(med[old_a] - med[old_b])
        best = min(med[old_a], med[old_b])
        return {"margin_ms": round(margin, 4), "new_over_old": round(med[new] / best, 4), "faster_by_more_than_the_margin": bool(best - med[new] > margin)}

    # ---- the decoder alone
    for n, k in CODES:
        rs = ctx.rs_create(n, k)
        src = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda", generator=g)
        pk = ctx.fec_rs_encode_packets_device(rs, src, 1, block0=0)   # straight order: symbol j of block b is packet b n + j
        lost = torch.rand((B, n), device="cuda", generator=g) < a.loss
        words = torch.arange(B * n, dtype=torch.int32, device="cuda").view(B, n).masked_fill(lost, -1)
        flags = lost.to(torch.uint8)
        sym = torch.empty((B, n, S), dtype=torch.uint8, device="cuda")
        payload = pk[:, 8:].view(B, n, S)
        out_r = (torch.empty((B, k, S), dtype=torch.uint8, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"),
                 torch.empty(B, dtype=torch.int32, device="cuda"))
        out_f = tuple(torch.empty_like(t) for t in out_r)
        sym.copy_(payload)
        ms = timed([("rs_decode_frames_a", lambda: ctx.rs_decode_frames(rs, sym, flags, out=out_f)),
                    ("rs_decode_rows", lambda: ctx.rs_decode_rows(rs, words, packets=pk, out=out_r)),
                    ("rs_decode_frames_b", lambda: ctx.rs_decode_frames(rs, sym, flags, out=out_f)),
                    ("gather", lambda: sym.copy_(payload))])
        entry = {name: stats(v) for name, v in ms.items()}
        decoded = out_f[2] == 0
        entry.update(verdict(ms, "rs_decode_rows", "rs_decode_frames_a", "rs_decode_frames_b"),
                     same_results=bool(all(torch.equal(x, y) for x, y in zip(out_r, out_f))), decoded=int(decoded.sum().item()),
                     source_recovered=bool(torch.equal(out_r[0][decoded], src[decoded])),
                     mean_missing_source_rows=round(float(lost[:, :k].sum(1).float().mean().item()), 2))
        res["decoder"]["rs%d_%d" % (n, k)] = entry
        del src, pk, lost, words, flags, sym, payload, out_r, out_f
        torch.cuda.empty_cache()

    # ---- whole receiver calls, RS(255,192)
    n, k = CODES[0]
    rs = ctx.rs_create(n, k)
    src = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda", generator=g)
    sent = ctx.fec_rs_encode_packets_device(rs, src, D, block0=0)
    pk = sent[torch.rand(B * n, device="cuda", generator=g) >= a.loss].contiguous()
    got = {}

    def one_call(name, knob):
        def run():
            ctx.configure("LDPC_AMD_RX_PKT", knob)
            try:
                with ctx.fec_rx_window(n, k, S, W, A, depth=D) as rx:
                    b, msg, received, status, used = rx.rs_decode_many(rs, pk, B)
                    got[name] = {"blocks": int(len(b)), "consumed": int(used), "decoded": int((status == 0).sum().item()),
                                 "info": ctx.fec_rs_receiver_info(), "msg": msg}
                    torch.cuda.synchronize()
            finally:
                ctx.configure("LDPC_AMD_RX_PKT", None)
        return run

    def two_calls(name):
        def run():
            with ctx.fec_rx_window(n, k, S, W, A, depth=D) as rx:
                b, sym, er, used = rx.push_many(pk, B)
                r = ctx.rs_decode_frames(rs, sym, er)
                got[name] = {"blocks": int(len(b)), "consumed": int(used), "decoded": int((r.status == 0).sum().item()), "msg": r.msg}
                torch.cuda.synchronize()
        return run

    ms = timed([("push_many_then_rs_decode_frames_a", two_calls("push_many_then_rs_decode_frames_a")), ("rs_decode_many_fused", one_call("rs_decode_many_fused", None)),
                ("rs_decode_many_composed", one_call("rs_decode_many_composed", 0)),
                ("push_many_then_rs_decode_frames_b", two_calls("push_many_then_rs_decode_frames_b"))])
    same = all(torch.equal(got["rs_decode_many_fused"]["msg"], v["msg"]) for v in got.values())
    res["receiver"] = {name: dict(stats(v), **{kd: x for kd, x in got[name].items() if kd != "msg"}) for name, v in ms.items()}
    res["receiver"].update(against_the_two_calls=verdict(ms, "rs_decode_many_fused", "push_many_then_rs_decode_frames_a", "push_many_then_rs_decode_frames_b"),
                           fused_over_composed=round(statistics.median(ms["rs_decode_many_fused"]) / statistics.median(ms["rs_decode_many_composed"]), 4),
                           same_msg=bool(same), packets=int(pk.shape[0]), window=[W, A, D],
                           note="whole calls, object creation and the host's read-backs included")
    del got, src, sent, pk
    ctx.close()
    torch.cuda.empty_cache()
    if a.parent_lib:
        res["sender"] = sender_ab(a.parent_lib, api.LIB_PATH, a.rounds, a.sender_blocks, S, a.steps, a.warmup)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
