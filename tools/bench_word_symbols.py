#!/usr/bin/env python3
"""Word-sized symbols (include/ldpc_erasure_amd_words.h) against the padded alternative, on one GPU: BASELINE cfg 2 -- the
(2040,1530) code, 4096 frames, 10 % uniform erasures -- at S = 1460 on a context with symbol unit 4 (the kernels' word form:
overlapped last piece, 4-byte accesses) and at S = 1472, the same symbols zero-padded to the next multiple of 16, on a default
context.  Same build, same box, one process; four operations each:

    decode     ctx.decode_frames, device tensors in and out
    encode     ctx.encode
    sender     ctx.fec_encode_packets_device (the fused sender)
    receiver   FecRxDevice.decode_many on a fresh receiver (the fused receiver), packets in transmission order, 10 % lost

The two lengths alternate step by step after a warm-up of each; every step is timed with device events.  Per operation: median
ms per step of either length, frames/s, and the ratio word / padded (below 1: the word form is faster than padding).

    python tools/bench_word_symbols.py [--frames 4096] [--steps 10] [--warmup 2] [--limit 600] [--out profiles/word_symbols_bench.json]

--limit: seconds after which the run gives up (exit status 124) instead of occupying the device.  One JSON line on stdout; --out
also writes it (indented) to a file."""
import argparse
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1460)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--loss", type=float, default=0.10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=600)
    ap.add_argument("--out")
    a = ap.parse_args()

    def give_up(*_):
        sys.stderr.write(f"bench_word_symbols: over the limit of {a.limit} s\n")
        os._exit(124)
    signal.signal(signal.SIGALRM, give_up)
    signal.alarm(a.limit)

    import torch
    from ldpc_erasure_codes_amd import api, codes
    F, S = a.frames, a.S
    Sp = (S + 15) & ~15
    assert S % 4 == 0 and S >= 16 and Sp != S, "--S: a multiple of 4 that is no multiple of 16"
    g = torch.Generator(device="cuda").manual_seed(11)
    sides = {}
    for name, s_, unit in (("word", S, 4), ("padded", Sp, 16)):
        ctx = api.Context(0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_symbol_unit(unit)
        h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
        n, k, _ = ctx.code_info(h)
        if name == "word":
            src = torch.randint(0, 256, (F, k, S), dtype=torch.uint8, device="cuda", generator=g)
            era = (torch.rand((F, n), device="cuda", generator=g) < a.loss).to(torch.uint8)
            order = torch.arange(F * n, device="cuda")[(era.reshape(-1) == 0)]
        else:                                                       # the same symbols, zero-padded
            w = sides["word"]
            src = torch.zeros((F, k, Sp), dtype=torch.uint8, device="cuda")
            src[:, :, :S] = w["src"]
        cw = ctx.encode(h, src)
        pk_all = ctx.fec_encode_packets_device(h, src, 1, 0)
        pk = pk_all[order].contiguous()                           # what the channel delivers: the erased symbols' packets are lost
        torch.cuda.synchronize()
        sym = cw.clone()
        sym[era.bool()] = 0
        sides[name] = dict(ctx=ctx, h=h, n=n, k=k, S=s_, src=src, cw=cw, sym=sym, pk=pk, pk_out=pk_all, last={}, paths={})
        del pk_all

    def op_decode(d):
        d["last"]["decode"] = d["ctx"].decode_frames(d["h"], d["sym"], era)

    def op_encode(d):
        d["ctx"].encode(d["h"], d["src"], out=d["cw"])

    def op_sender(d):
        d["ctx"].fec_encode_packets_device(d["h"], d["src"], 1, 0, out=d["pk_out"])
        d["paths"]["sender"] = d["ctx"].fec_sender_info()["path"]

    def op_receiver(d):
        rx = d["ctx"].fec_rx_device(d["n"], d["k"], d["S"])
        d["last"]["receiver"] = rx.decode_many(d["h"], d["pk"], F)
        d["paths"]["receiver"] = d["ctx"].fec_receiver_info()["path"]
        torch.cuda.synchronize()
        rx.close()

    ops = (("decode", op_decode), ("encode", op_encode), ("sender", op_sender), ("receiver", op_receiver))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def step(fn, d, timed):
        torch.cuda.synchronize()
        ev[0].record()
        fn(d)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) if timed else None

    # both lengths give the same bytes (checked once, on the whole batch): the computation is columnwise
    for nm, fn in ops:
        for d in sides.values():
            step(fn, d, False)
    w, p = sides["word"], sides["padded"]
    assert torch.equal(w["cw"], p["cw"][:, :, :S]) and torch.equal(w["pk_out"][:, 8:], p["pk_out"][:, 8:8 + S])
    fw, fp = w["last"]["decode"], p["last"]["decode"]
    assert torch.equal(fw.out, fp.out[:, :, :S]) and all(torch.equal(x, y) for x, y in zip(fw[1:], fp[1:]))
    (bw, rw, uw), (bp, rp, up) = w["last"]["receiver"], p["last"]["receiver"]
    assert uw == up and (bw == bp).all() and torch.equal(rw.out, rp.out[:, :, :S]) and all(torch.equal(x, y) for x, y in zip(rw[1:], rp[1:]))
    status = fw.status.cpu().numpy()
    blocks = int(len(bw))
    for d in sides.values():
        d["last"].clear()
    torch.cuda.empty_cache()

    ms = {nm: {"word": [], "padded": []} for nm, _ in ops}
    for nm, fn in ops:
        for _ in range(a.warmup):
            for d in sides.values():
                step(fn, d, False)
                d["last"].clear()
        for _ in range(a.steps):
            for side, d in sides.items():
                ms[nm][side].append(step(fn, d, True))
                d["last"].clear()
    res = {"device": torch.cuda.get_device_name(0), "code": [w["n"], w["k"]], "frames": F, "loss": a.loss, "S_word": S, "S_padded": Sp,
           "padding_saved_pct": round(100.0 * (Sp - S) / Sp, 2), "steps": a.steps, "receiver_blocks_per_step": blocks,
           "frames_decoded_by_message_passing": int((status == 0).sum()),
           "kernels_word": w["ctx"].profile_kernel_names(), "kernels_padded": p["ctx"].profile_kernel_names(),
           "paths_word": w["paths"], "paths_padded": p["paths"], "ops": {}}
    for nm, v in ms.items():
        mw, mp = statistics.median(v["word"]), statistics.median(v["padded"])
        per = blocks if nm == "receiver" else F
        res["ops"][nm] = {"word_ms": round(mw, 4), "padded_ms": round(mp, 4), "word_min_max_ms": [round(min(v["word"]), 4), round(max(v["word"]), 4)],
                          "padded_min_max_ms": [round(min(v["padded"]), 4), round(max(v["padded"]), 4)],
                          "word_frames_per_s": round(per / (mw * 1e-3), 1), "padded_frames_per_s": round(per / (mp * 1e-3), 1),
                          "word_over_padded": round(mw / mp, 3)}
    for d in sides.values():
        d["ctx"].close()
    signal.alarm(0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
