#!/usr/bin/env python3
"""The datagram calls (include/ldpc_erasure_amd_datagrams.h) on one GPU, BASELINE cfg 2 shape: the (2040,1530) code at S = 1024,
4096 frames of the reference's datagram mix (tools/datagram_frames.difi_mix: one 112-byte context datagram per 16 data datagrams
of S - 4 bytes).

    pack            Context.fec_pack_datagrams: datagrams back to back -> source [F][k][S]
    unpack          Context.fec_unpack_datagrams on decoded frames [F][n][S] with their flags
    encode          Context.fec_encode_packets_device on the pre-padded source (what a caller with fixed-length symbols runs)
    pack+encode     pack, then the same encode
    decode          FecRxDevice.decode_many over the lossy packet stream (a fresh receiver per step)
    decode+unpack   the same, then unpack of its frames
    copy            Context.copy_probe over F k S bytes: the yardstick -- the same bytes written and no fewer read

The timed variants alternate step by step in ONE process, after a warm-up of each, device events around every step; median ms.
Beside each step's time: the wall-clock time until its calls had returned, their host part (pack checks and stages N + 1 offsets).
Recorded: pack / copy and unpack / copy, and what pack and unpack add to the calls they stand beside.  Before timing, pack is
checked against the numpy model on the first frames and unpack(pack(x)) against x on all of them.

    python tools/bench_datagrams.py [--frames 4096] [--steps 10] [--warmup 2] [--loss 0.05] [--out profiles/datagrams_bench.json]

One JSON line on stdout; --out also writes it (indented) to a file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def summary(v):
    return {"ms_per_step_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--code", type=int, default=1)
    ap.add_argument("--loss", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from ldpc_erasure_codes_amd import api, codes
    import datagram_frames as dg
    F, S = a.frames, a.S
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = ctx.load_builtin_code(a.code, codes.DEFAULT_COEF_SEED[a.code])
    n, k, _ = ctx.code_info(h)
    N = F * k
    gen = torch.Generator(device="cuda").manual_seed(5)
    # the mix: lengths on the host (they are the call's host argument), contents drawn on the device
    ln = np.full(N, S - dg.PREFIX, dtype=np.int64)
    ln[::17] = dg.CONTEXT_BYTES
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    data = torch.randint(0, 256, (int(off[-1]),), dtype=torch.uint8, device="cuda", generator=gen)
    source = torch.empty((F, k, S), dtype=torch.uint8, device="cuda")
    packets = torch.empty((F * n, 8 + S), dtype=torch.uint8, device="cuda")

    # pack against the model (first frames), then the round trip on everything
    ctx.fec_pack_datagrams(data, off, k, S, out=source)
    torch.cuda.synchronize()
    head = 2 * k
    if not np.array_equal(source[:2].cpu().numpy(), dg.pack(data[:int(off[head])].cpu().numpy(), off[:head + 1], k, S)):
        raise SystemExit("pack differs from the model")
    rt = ctx.fec_unpack_datagrams(source, k)
    torch.cuda.synchronize()
    if not (torch.equal(rt.offset, torch.from_numpy(off).cuda()) and torch.equal(rt.bytes[:data.shape[0]], data) and int(rt.state.max()) == 0):
        raise SystemExit("unpack(pack(x)) differs from x")
    del rt

    # the receiver's input: the packets of that source, uniform loss, transmission order
    ctx.fec_encode_packets_device(h, source, 1, 0, out=packets)
    torch.cuda.synchronize()
    keep = torch.rand(F * n, device="cuda", generator=gen) >= a.loss
    kept = packets[keep].contiguous()
    del keep
    last = {}

    def run_pack():
        ctx.fec_pack_datagrams(data, off, k, S, out=source)

    def run_encode():
        ctx.fec_encode_packets_device(h, source, 1, 0, out=packets)

    def run_pack_encode():
        run_pack()
        run_encode()

    def run_decode(rx):
        last["fr"] = rx.decode_many(h, kept, F, out=last.get("buf"))

    def run_decode_unpack(rx):
        run_decode(rx)
        fr = last["fr"][1]
        last["dg"] = ctx.fec_unpack_datagrams(fr.out, k, fr.erased_out)

    rx0 = ctx.fec_rx_device(n, k, S)
    last["buf"] = rx0._frames(F)   # the decoder's outputs, allocated once and reused by every step
    run_decode(rx0)
    torch.cuda.synchronize()
    blocks, fr, used = last["fr"]
    closes = int(len(blocks))
    frames_out, flags_out = fr.out, fr.erased_out
    rx0.close()
    # unpack behind the decoder: everything the decoder recovered is the datagram that was sent
    got = ctx.fec_unpack_datagrams(frames_out, k, flags_out)
    torch.cuda.synchronize()
    st = got.state.cpu().numpy()
    lost_rows = int((st == api.DGRAM_LOST).sum())
    if int((st == api.DGRAM_MALFORMED).sum()) or int((st == api.DGRAM_FILLER).sum()):
        raise SystemExit("decoded frames hold rows that are not datagram symbols")
    o = got.offset.cpu().numpy()
    want_len = np.where(st == api.DGRAM_DELIVERED, ln[:closes * k], 0)
    if not np.array_equal(np.diff(o), want_len):
        raise SystemExit("unpack behind the decoder: lengths differ from what was sent")
    del got

    def run_unpack():
        last["dg"] = ctx.fec_unpack_datagrams(frames_out, k, flags_out)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(body, with_rx=False):
        rx = ctx.fec_rx_device(n, k, S) if with_rx else None   # a fresh receiver: every step sees the stream from its first packet
        torch.cuda.synchronize()
        ev[0].record()
        t0 = time.perf_counter()
        body(rx) if with_rx else body()
        host = (time.perf_counter() - t0) * 1e3   # until the calls have returned: their host part (everything behind it is enqueued)
        ev[1].record()
        torch.cuda.synchronize()
        if rx:
            rx.close()
        last.pop("dg", None)
        return ev[0].elapsed_time(ev[1]), host

    variants = (("pack", run_pack, False), ("unpack", run_unpack, False), ("encode", run_encode, False), ("pack+encode", run_pack_encode, False),
                ("decode", run_decode, True), ("decode+unpack", run_decode_unpack, True))
    for _ in range(a.warmup):
        for _, fn, w in variants:
            timed(fn, w)
    ms = {nm: [] for nm, _, _ in variants}
    host_ms = {nm: [] for nm, _, _ in variants}
    for _ in range(a.steps):
        for nm, fn, w in variants:
            t, hst = timed(fn, w)
            ms[nm].append(t)
            host_ms[nm].append(hst)
    med = {nm: statistics.median(v) for nm, v in ms.items()}
    hmed = {nm: statistics.median(v) for nm, v in host_ms.items()}
    info = ctx.fec_dgram_info()
    last.clear()
    del frames_out, flags_out, fr
    torch.cuda.empty_cache()
    # the yardstick, in the same run: a streaming copy of F k S bytes (source -> the packet array's memory)
    nbytes = F * k * S
    copy_ms = ctx.copy_probe(source.view(-1), packets.view(-1), reps=a.steps, nbytes=nbytes)
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "datagrams": N, "datagram_bytes": int(off[-1]),
           "context_datagrams": int((ln == dg.CONTEXT_BYTES).sum()), "loss": a.loss, "blocks_closed_per_step": closes, "rows_lost_behind_the_decoder": lost_rows,
           "steps": a.steps, "warmup": a.warmup, "knobs": ctx.knobs(), "sender_path": ctx.fec_sender_info()["path"],
           "receiver_path": ctx.fec_receiver_info()["path"], "dgram_info": info,
           "variants": {nm: dict(summary(v), host_ms_median=round(hmed[nm], 4)) for nm, v in ms.items()},
           "copy_probe": {"bytes": nbytes, "ms_best": round(copy_ms, 4), "TBps_read_plus_write": round(2 * nbytes / (copy_ms * 1e-3) / 1e12, 3)},
           "pack_over_copy": round(med["pack"] / copy_ms, 3), "unpack_over_copy": round(med["unpack"] / copy_ms, 3),
           # a step is the host part of its calls (for pack: checking and staging N + 1 offsets), then what they enqueued
           "pack_behind_host_ms": round(med["pack"] - hmed["pack"], 4), "pack_behind_host_over_copy": round((med["pack"] - hmed["pack"]) / copy_ms, 3),
           "pack_TBps_read_plus_write": round((int(off[-1]) + nbytes) / (med["pack"] * 1e-3) / 1e12, 3),
           "unpack_TBps_read_plus_write": round(2 * int(off[-1]) / (med["unpack"] * 1e-3) / 1e12, 3),
           "pack+encode_over_encode": round(med["pack+encode"] / med["encode"], 3),
           "pack_added_ms": round(med["pack+encode"] - med["encode"], 4),
           "decode+unpack_over_decode": round(med["decode+unpack"] / med["decode"], 3),
           "unpack_added_ms": round(med["decode+unpack"] - med["decode"], 4)}
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
