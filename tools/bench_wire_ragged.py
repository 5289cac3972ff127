#!/usr/bin/env python3
"""The trimmed wire (include/ldpc_erasure_amd_wire_ragged.h) on one GPU, BASELINE cfg 2 shape: the (2040,1530) code at S = 1024,
4096 frames of the reference's datagram mix (tools/datagram_frames.difi_mix: one 112-byte context datagram per 16 data datagrams
of S - 4 bytes), packed and sent by the fused sender: P = F n packets of 8 + S bytes.

    trim      Context.fec_trim_packets: the packet array -> the wire bytes back to back and their offsets
    land      Context.fec_land_packets: those bytes and offsets -> a packet array, zero fill included
    unpack    Context.fec_unpack_datagrams on the packed source [F][k][S], nothing erased (trim's launch structure)
    pack      Context.fec_pack_datagrams: the datagrams -> source [F][k][S] (land's launch structure, plus its host-side offsets)
    copy      Context.copy_probe over P (8 + S) bytes: the yardstick -- no fewer bytes written, no fewer read

The timed variants alternate step by step in ONE process, after a warm-up of each, device events around every step; median ms.
Recorded: trim / copy, land / copy, trim / unpack, land / pack, and for trim and unpack the time per byte moved (read + written)
with the repeat-to-repeat spread of each.  Before timing, trim's lengths are checked against ldpc_amd_fec_dgram_wire_len and
land(trim(x)) against x.

    python tools/bench_wire_ragged.py [--frames 4096] [--steps 10] [--warmup 2] [--out profiles/wire_ragged_bench.json]

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
    N, P, plen = F * k, F * n, 8 + S
    gen = torch.Generator(device="cuda").manual_seed(5)
    # the mix: lengths on the host (pack's host argument), contents drawn on the device
    ln = np.full(N, S - dg.PREFIX, dtype=np.int64)
    ln[::17] = dg.CONTEXT_BYTES
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    data = torch.randint(0, 256, (int(off[-1]),), dtype=torch.uint8, device="cuda", generator=gen)
    source = torch.empty((F, k, S), dtype=torch.uint8, device="cuda")
    packets = torch.empty((P, plen), dtype=torch.uint8, device="cuda")
    ctx.fec_pack_datagrams(data, off, k, S, out=source)
    ctx.fec_encode_packets_device(h, source, 1, 0, out=packets)
    wire = api.Wire(torch.empty(P * plen, dtype=torch.uint8, device="cuda"), torch.empty(P + 1, dtype=torch.int64, device="cuda"))
    landed = torch.empty((P, plen), dtype=torch.uint8, device="cuda")

    # trim's lengths against the host arithmetic, then the round trip on everything
    ctx.fec_trim_packets(packets, k, out=wire)
    torch.cuda.synchronize()
    wl = torch.from_numpy(api.fec_datagram_wire_len(off, n, k, S).astype(np.int64)).cuda()
    if not torch.equal(wire.offset[1:] - wire.offset[:-1], wl):
        raise SystemExit("trim's lengths differ from ldpc_amd_fec_dgram_wire_len")
    total = int(wire.offset[-1])
    del wl
    _, st = ctx.fec_land_packets(wire.bytes, wire.offset, S, out=landed)
    torch.cuda.synchronize()
    if int(st.max()) != api.WIRE_LANDED:
        raise SystemExit("land rejected a datagram trim made")
    step = 1 << 20
    for p0 in range(0, P, step):
        if not torch.equal(landed[p0:p0 + step], packets[p0:p0 + step]):
            raise SystemExit("land(trim(x)) differs from x")
    del st
    last = {}

    def run_trim():
        ctx.fec_trim_packets(packets, k, out=wire)

    def run_land():
        last["st"] = ctx.fec_land_packets(wire.bytes, wire.offset, S, out=landed)[1]

    def run_unpack():
        last["dg"] = ctx.fec_unpack_datagrams(source, k)

    def run_pack():
        ctx.fec_pack_datagrams(data, off, k, S, out=source)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(body):
        torch.cuda.synchronize()
        ev[0].record()
        t0 = time.perf_counter()
        body()
        host = (time.perf_counter() - t0) * 1e3   # until the calls have returned: their host part (everything behind it is enqueued)
        ev[1].record()
        torch.cuda.synchronize()
        last.clear()
        return ev[0].elapsed_time(ev[1]), host

    variants = (("trim", run_trim), ("land", run_land), ("unpack", run_unpack), ("pack", run_pack))
    for _ in range(a.warmup):
        for _, fn in variants:
            timed(fn)
    ms = {nm: [] for nm, _ in variants}
    host_ms = {nm: [] for nm, _ in variants}
    for _ in range(a.steps):
        for nm, fn in variants:
            t, hst = timed(fn)
            ms[nm].append(t)
            host_ms[nm].append(hst)
    med = {nm: statistics.median(v) for nm, v in ms.items()}
    hmed = {nm: statistics.median(v) for nm, v in host_ms.items()}
    info = ctx.fec_wire_ragged_info()
    torch.cuda.empty_cache()
    # the yardstick, in the same run: a streaming copy of P (8 + S) bytes (the packet array -> the wire buffer)
    nbytes = P * plen
    copy_ms = ctx.copy_probe(packets.view(-1), wire.bytes, reps=a.steps, nbytes=nbytes)
    # time per byte moved (read + written): trim moves the wire bytes twice, unpack the datagram bytes twice (prefixes and lengths aside)
    moved = {"trim": 2 * total, "unpack": 2 * int(off[-1])}
    ps = {nm: {"median": round(med[nm] * 1e9 / moved[nm], 4), "min": round(min(ms[nm]) * 1e9 / moved[nm], 4), "max": round(max(ms[nm]) * 1e9 / moved[nm], 4)}
          for nm in moved}
    res = {"device": torch.cuda.get_device_name(0), "code": [n, k], "S": S, "frames": F, "packets": P, "packet_bytes": nbytes, "wire_bytes": total,
           "wire_over_packet_bytes": round(total / nbytes, 4), "datagrams": N, "datagram_bytes": int(off[-1]), "steps": a.steps, "warmup": a.warmup,
           "knobs": ctx.knobs(), "sender_path": ctx.fec_sender_info()["path"], "wire_ragged_info": info,
           "variants": {nm: dict(summary(v), host_ms_median=round(hmed[nm], 4)) for nm, v in ms.items()},
           "copy_probe": {"bytes": nbytes, "ms_best": round(copy_ms, 4), "TBps_read_plus_write": round(2 * nbytes / (copy_ms * 1e-3) / 1e12, 3)},
           "trim_over_copy": round(med["trim"] / copy_ms, 3), "land_over_copy": round(med["land"] / copy_ms, 3),
           "trim_over_unpack": round(med["trim"] / med["unpack"], 3), "land_over_pack": round(med["land"] / med["pack"], 3),
           "unpack_over_copy": round(med["unpack"] / copy_ms, 3), "pack_over_copy": round(med["pack"] / copy_ms, 3),
           "trim_TBps_read_plus_write": round(2 * total / (med["trim"] * 1e-3) / 1e12, 3),
           "land_TBps_read_plus_write": round((total + nbytes) / (med["land"] * 1e-3) / 1e12, 3),
           "unpack_TBps_read_plus_write": round(2 * int(off[-1]) / (med["unpack"] * 1e-3) / 1e12, 3),
           "picoseconds_per_byte_moved": ps,
           # trim is slower per byte moved than unpack by more than the repeat-to-repeat spread when even its fastest step is behind unpack's slowest
           "trim_slower_per_byte_than_unpack_beyond_spread": bool(ps["trim"]["min"] > ps["unpack"]["max"])}
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
