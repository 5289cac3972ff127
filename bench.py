#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric, measured on one MI355X per process.

Headline (`value`): BASELINE configs[1] = cfg 2:

    decoded frames/sec + recovered GB/s, n=2040 k=1530 GF(256) LDPC, 10 % uniform random erasures,
    batch = 4096 frames per GPU, hybrid MP + ML decoder (max 10 sweeps, ML armed).

A "step" is one pass of the hot path (ldpc_amd_decode_batch: peel -> packet kernel -> ML stage on the residual frames)
over one batch of synthetic frames already resident in HBM when the timed region starts.  Symbols are S-byte packets
(--S, default 1024 = the reference's FPGA packet, OpenCL/host/src/main.cpp:42-47); the Matlab-exact scalar case S = 1 is
measured in the same run and reported under "s1".  At 10 % erasures the ML stage is armed but never triggers (the
line says so: ml_trigger_rate); the configs that exercise it are in the "configs" block of the same JSON line:

    cfg3  (2040,1530) hybrid MP+ML, Gilbert-Elliott erasures pushed until the ML stage triggers on >= 10 % of the frames
          (SURVEY.md 8d), S = 1024 and S = 1
    cfg4  (4080,3060) [synthesised matrix] vs 16 x RS(255,223) on the same erasure patterns, 65536 frames, S = 1
          + cfg4_S1024: the same code and RS(255,223) in packet mode (S = 1024), the first 4096 frames of that stream
          (alone: `--full --config 4 --S 1` / `--full --config 4 --S 1024`)
    cfg5  mixed (4000,2000) + (2040,1530) stream, 1:1, 10 % -- at N = 1 the whole 65536-frame stream (the strong-scaling anchor),
          one GPU's 1/8 share, and an S = 64 run whose final gather moves the decoded outputs

each with frames/s, per-kernel ms (HIP events inside the library, on the launch stream), algorithmic bytes,
the roofline fraction they give, ML-trigger / rank-deficient rates and a bounded CPU-baseline sample of the same inputs.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    ... bench.py --full --gpus 8 --config 5 --gather outputs      # BASELINE configs[4] on an 8-GPU node (strong scaling)

One process per GPU; frames are sharded with no data-path collective (cfg 2: weak scaling, 4096 frames per GPU; cfg 5:
the 65536-frame mixed stream split over the ranks); RCCL is used once, for the final gather (status words, or outputs +
status words with --gather outputs).  Rank 0 prints ONE JSON line.

The oracle (oracle/) is used here only (a) to time the CPU baseline and (b) to spot-check decoded frames after the timed
region; the measured path is the HIP library behind the C ABI.

A plain run (`--gpus N --steps K --warmup W`) does only what the headline needs: it sets up the cfg 2 batch at --S, runs W
untimed and K timed steps and prints the line (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, ...).
Everything described above besides that -- the S = 1 companion run, the CPU baselines, the cfg 3/4/5 block (or `--config
3/4/5` alone), the sustained / pipelined / encoder / in-place / copy-probe / xGMI figures, the replayed PMC roofline, the
oracle spot checks and the detail file (--detail-out) -- runs with `--full`.

`--dump-outputs DIR` writes what the timed path returned in its last headline step as float32 .npy files (dump_outputs):
two builds given the same arguments decode the same seeded inputs and can be compared output for output.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md: 8 TB/s; ~6.3 TB/s achievable)
SEED_SRC, SEED_ERA = 20261004, 20261005
GE_PARAMS = (0.13, 0.8, 10.0)   # cfg 3: alpha, beta, good_transition_bias -- ML stage on ~28 % of the frames
# PMC summaries (separate rocprofv3 --pmc passes of this same command, committed): newest first
PMC_SUMMARIES = [os.path.join(ROOT, "profiles", f) for f in
                 ("round4_pmc_summary.json", "round4_cfg4p_pmc_summary.json", "round3_pmc_summary.json", "round3_cfg4p_pmc_summary.json", "round2_pmc_summary.json")]

# BASELINE.json configs -> (code_ind, channel, frames)
WORKLOADS = {
    "cfg2": dict(code=1, channel=("uniform", 0.10), frames=4096),
    "cfg3": dict(code=1, channel=("bursty",) + GE_PARAMS, frames=4096),
    "cfg4": dict(code=3, channel=("uniform", 0.10), frames=65536, rs=(255, 223)),
    # cfg 4's code on the packet (HBM-roofline) path: 65536 frames x 4080 x 1 KB x 2 would be 548 GB, so the packet run takes
    # the first 4096 frames of the same stream (34 GB in + out)
    "cfg4p": dict(code=3, channel=("uniform", 0.10), frames=4096),
    "cfg5": dict(codes=(2, 1), channel=("uniform", 0.10), frames=65536),
}


DUMP_SEED, DUMP_FRAMES, DUMP_LANES = 20261016, 256, 16   # --dump-outputs: the fixed sample of the decoded symbols
DUMP_LIMIT_BYTES = 64 << 20


def alg_bytes_per_frame(n, S):
    # symbols in + erasure flags in + Msg out + sweeps/residual words
    return 2 * n * S + n + 8


def rs_alg_bytes_per_block(k, S):
    # k*S in + 2k (indices) + k*S out
    return 2 * k * S + 2 * k


def pmc_traffic(kernel, workload="cfg2"):
    """(HBM bytes per launch of `kernel`, source file) from the committed rocprofv3 PMC summaries (separate --pmc FETCH_SIZE /
    WRITE_SIZE passes of this same command, gfx950 correction applied: tools/summarize_profiles.py).  The counters cannot be
    read from inside this process, so the figure is REPLAYED from the committed file of the same workload and kernel name (the
    line says which: roofline.traffic_source); a launch plan no summary knows gets a warning, not a silent null."""
    seen = []
    for path in PMC_SUMMARIES:
        if not os.path.exists(path):
            continue
        try:
            doc = json.load(open(path))
            ks = doc["kernels"]
        except (KeyError, ValueError):
            continue
        if doc.get("workload", "cfg2") != workload:
            continue
        seen += sorted(ks)
        if kernel in ks and ks[kernel].get("traffic_bytes") is not None:
            return ks[kernel]["traffic_bytes"], os.path.relpath(path, ROOT) + " (replayed: separate --pmc passes of this command)"
    print(f"bench.py: no committed PMC summary of workload {workload} has the launched kernel '{kernel}' (have: {seen}): "
          "roofline.traffic = null -- re-run the --pmc passes for this launch plan", file=sys.stderr)
    return None, None


# ----------------------------------------------------------------------------------------------------
# CPU baseline ("port": oracle/oracle.c, the line-faithful restatement of the Matlab decoders), run BEFORE the GPU is
# touched so that forked workers never inherit a HIP context.  Every worker decodes frames of the SAME batch the GPU
# decodes (same seeds, same frame indices; worker w takes frames w, w + W, ...) for a bounded time.
# ----------------------------------------------------------------------------------------------------
def host_erasures(cfg, code_ind, n, nframes, frame0=0):
    from oracle import oracle_py
    ch = WORKLOADS[cfg]["channel"]
    if ch[0] == "uniform":
        return oracle_py.synth_erasures_uniform(SEED_ERA + code_ind, frame0, nframes, n, ch[1])
    return oracle_py.synth_erasures_bursty(SEED_ERA + code_ind, frame0, nframes, n, ch[1], ch[2], ch[3])


def _cpu_worker(args):
    wid, nworkers, cfg, S, seconds = args
    from ldpc_erasure_codes_amd import codes, synth
    from oracle import oracle_py
    w = WORKLOADS[cfg]
    code_inds = w.get("codes", (w.get("code"),))
    F = w["frames"]
    ocs, eras = {}, {}
    for ci in code_inds:
        c = codes.load_builtin(ci)
        ocs[ci] = (c, oracle_py.OracleCode(c))
        if cfg == "cfg3":
            eras[ci] = host_erasures(cfg, ci, c.n, F)   # the GE chain is sequential: the whole batch, once
    rs_g = oracle_py.rs_generator(*w["rs"]) if "rs" in w else None
    busy = busy_rs = 0.0
    frames = blocks = ml = 0
    f = wid
    chunk = 64 if S == 1 else 2
    while busy + busy_rs < seconds:
        # worker w takes frames w, w + W, ... of the GPU's batch and starts over at the end (on a many-core host the batch is
        # only a few frames per worker; every worker still decodes for the stated time)
        ids = [(f + i * nworkers) % F for i in range(chunk)]
        f = (ids[-1] + nworkers) % F
        for ci in code_inds:
            c, oc = ocs[ci]
            mine = [g for g in ids if len(code_inds) == 1 or (g % len(code_inds)) == code_inds.index(ci)]
            if not mine:
                continue
            if cfg == "cfg3":
                era = eras[ci][mine]
            else:
                era = np.concatenate([host_erasures(cfg, ci, c.n, 1, g) for g in mine])
            keep = era.sum(axis=1) < c.m       # Matlab harness: decoder called only if num_erasures < n-k (...Sim.m:216)
            era = np.ascontiguousarray(era[keep])
            mine = [g for g, kp in zip(mine, keep) if kp]
            if not mine:
                continue
            src = np.concatenate([oracle_py.synth_source(SEED_SRC + ci, g, 1, c.k, S) for g in mine])
            if S == 1:
                cw = np.stack([oc.encode(src[i, :, 0]) for i in range(len(mine))])
                t0 = time.perf_counter()
                out, sw, res, st = oc.decode_batch_s1(cw, era)
                busy += time.perf_counter() - t0
                okf = st <= 1
                assert np.array_equal(out[okf], cw[okf])
                ml += int((res > 0).sum())
            else:
                cws = [oc.encode(src[i]) for i in range(len(mine))]
                t0 = time.perf_counter()
                outs = [oc.decode_packets(cws[i], era[i]) for i in range(len(mine))]
                busy += time.perf_counter() - t0
                ml += sum(int(o[3][0] > 0) for o in outs)
            frames += len(mine)
            if rs_g is not None:
                rn, rk = w["rs"]
                for i in range(len(mine)):
                    for b in range(c.n // rn):
                        recv = np.nonzero(era[i, b * rn:(b + 1) * rn] == 0)[0]
                        if recv.size < rk:
                            continue      # RS decode attempted only for blocks with >= k received (SURVEY 8d cfg 4)
                        idx = recv[:rk].astype(np.uint16)
                        rsrc = oracle_py.synth_source(SEED_SRC + 77, mine[i] * 16 + b, 1, rk, 1)[0, :, 0]
                        rcw = oracle_py.rs_encode(rs_g, rsrc)
                        t0 = time.perf_counter()
                        msg, _ = oracle_py.rs_decode(rs_g, idx, np.ascontiguousarray(rcw[idx]))
                        busy_rs += time.perf_counter() - t0
                        assert np.array_equal(msg, rsrc)
                        blocks += 1
    return frames, busy, blocks, busy_rs, ml


def cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg, S, seconds):
    """single_thread (one worker) and all_cores (one worker per core of this process's affinity mask)."""
    cores_total = len(os.sched_getaffinity(0))   # hardware THREADS of the affinity mask (SMT siblings count)
    out = {"unit": "frames/s", "kind": "port", "threads_total": cores_total, "cores_total": cores_total,
           "cores_total_note": "hardware threads of this process's affinity mask (SMT siblings included), one worker each",
           "cpu_model": cpu_model()}
    for label, nw in (("single_thread", 1), ("all_cores", min(cores_total, 256))):
        t0 = time.perf_counter()
        with mp.get_context("fork").Pool(nw) as pool:
            res = pool.map(_cpu_worker, [(w, nw, cfg, S, seconds if nw > 1 else 0.5 * seconds) for w in range(nw)])
        wall = time.perf_counter() - t0
        rate = sum(fr / b for fr, b, _, _, _ in res if b > 0)   # workers run concurrently: aggregate = sum of rates
        out[label] = rate
        frames = sum(r[0] for r in res)
        if label == "all_cores":
            if S >= 256 and out.get("single_thread"):
                out["all_cores_note"] = (f"{rate / out['single_thread']:.1f}x one thread on {nw} threads: at S={S} every worker streams "
                                         "MBs per frame, so the all-threads leg is bound by host memory bandwidth, not by cores")
            out.update({"value": rate, "cores": nw,
                        "sample": f"{frames} frames of the GPU's own batch ({cfg}, S={S}) decoded by oracle/oracle.c, "
                                  f"~{seconds:g} s of decode time per worker on {nw} workers ({wall:.1f} s wall incl. input "
                                  f"generation and encoding); single_thread = the same with one worker",
                        "ml_frames_in_sample": sum(r[4] for r in res)})
            blocks = sum(r[2] for r in res)
            if blocks:
                out["rs_blocks_per_s"] = sum(bl / b for _, _, bl, b, _ in res if b > 0)
                out["rs_blocks_in_sample"] = blocks
        elif sum(r[2] for r in res):
            out["rs_blocks_per_s_single_thread"] = sum(bl / b for _, _, bl, b, _ in res if b > 0)
    return out


def cpu_cfg1(reps=200):
    """BASELINE configs[0] (the reference's own CPU-runnable case): ONE binary (2040,1530) frame, message passing only
    (Matlab/My_LDPC_Erasure_Decoder.m, 50 sweeps max), FPGA data_in erasures at PER 9/64 -- the oracle on one core."""
    from ldpc_erasure_codes_amd import codes, synth
    from oracle import oracle_py
    code = codes.load_builtin(1, 0)  # coefficient seed 0 = the binary code (all ones)
    oc = oracle_py.OracleCode(code)
    era = synth.fpga_erasures(1, 9, reps, code.n)
    busy, ok, sweeps = 0.0, 0, 0
    for f in range(reps):
        recv = np.zeros(code.n, dtype=np.int16)  # the all-zero codeword, as the FPGA source sends (data_in)
        recv[era[f] != 0] = -1
        t0 = time.perf_counter()
        msg, it = oc.binary_mp(recv, itenum=50)
        busy += time.perf_counter() - t0
        ok += int(not (msg < 0).any())
        sweeps += it
    return {"workload": "BASELINE cfg1: 1 binary (2040,1530) frame, MP only (<= 50 sweeps), PER 9/64, oracle on 1 core",
            "us_per_frame": busy / reps * 1e6, "frames": reps, "decoded": ok, "mean_sweeps": sweeps / reps}


# ----------------------------------------------------------------------------------------------------
# GPU side
# ----------------------------------------------------------------------------------------------------
class Gpu:
    def __init__(self, args, rank, world, local_rank):
        import torch
        import torch.distributed as dist
        from ldpc_erasure_codes_amd import api
        self.torch, self.dist = torch, dist
        self.args, self.rank, self.world = args, rank, world
        # LDPC_BENCH_BACKEND=gloo is only for rehearsing the N > 1 launch path on a box with fewer GPUs than ranks
        self.backend = os.environ.get("LDPC_BENCH_BACKEND", "nccl")
        if self.backend == "gloo":
            local_rank = local_rank % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local_rank)
        self.dev = torch.device("cuda", local_rank)
        if world > 1:
            if self.backend == "gloo":
                dist.init_process_group("gloo")
            else:
                dist.init_process_group("nccl", device_id=self.dev)
        self.ctx = api.Context(local_rank)
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)  # torch events and our kernels share one stream
        self.ctx.selftest()
        self.handles = {}

    def close(self):
        self.ctx.close()
        if self.world > 1:
            self.dist.destroy_process_group()

    def code(self, code_ind):
        from ldpc_erasure_codes_amd import codes
        if code_ind not in self.handles:
            h = self.ctx.load_builtin_code(code_ind, codes.DEFAULT_COEF_SEED[code_ind])
            self.handles[code_ind] = (h,) + tuple(self.ctx.code_info(h)[:2])
        return self.handles[code_ind]

    def barrier(self):
        if self.world > 1:
            self.dist.barrier()
        self.torch.cuda.synchronize()

    def make_batch(self, cfg, code_ind, S, frame_ids=None, frame0=0, nframes=None):
        """Codewords, received symbols and erasure flags, generated and encoded on the device.  frame_ids: explicit global
        frame indices (mixed stream); else frames [frame0, frame0 + nframes)."""
        torch, ctx = self.torch, self.ctx
        h, n, k = self.code(code_ind)
        ch = WORKLOADS[cfg]["channel"]
        if frame_ids is not None:
            # frames of a mixed stream are not contiguous in the per-frame generators' index space: generate the covering
            # range and pick (cheap: S = 1)
            lo, hi = (int(frame_ids.min()), int(frame_ids.max()) + 1) if len(frame_ids) else (0, 0)
            sel = torch.from_numpy(np.asarray(frame_ids) - lo).to(self.dev)
            frame0, nframes = lo, hi - lo
        F = nframes
        src = torch.empty((F, k, S), dtype=torch.uint8, device=self.dev)
        ctx.synth_source(SEED_SRC + code_ind, frame0, F, k, S, src)
        era = torch.empty((F, n), dtype=torch.uint8, device=self.dev)
        if ch[0] == "uniform":
            ctx.synth_erasures_uniform(SEED_ERA + code_ind, frame0, F, n, ch[1], era)
        else:
            ctx.synth_erasures_bursty(SEED_ERA + code_ind, frame0, F, n, ch[1], ch[2], ch[3], era)
        if frame_ids is not None:
            src, era = src[sel].contiguous(), era[sel].contiguous()
        keep = era.sum(dim=1, dtype=torch.int32) < (n - k)   # harness guard: decoder called only if E0 < n-k (...Sim.m:216)
        if not bool(keep.all()):
            src, era = src[keep].contiguous(), era[keep].contiguous()
        cw = ctx.encode(h, src if S > 1 else src.reshape(src.shape[0], k))
        del src
        sym = cw.clone()
        sym[era.bool()] = 0x5A  # the payload of an erased symbol is garbage, never the true value
        return cw, sym, era, keep

    def time_decode(self, h, sym, era, steps, warmup, after_steps=None, detail=False):
        """W untimed + K timed decode steps bracketed by barrier + synchronize; per-kernel HIP-event times from the library."""
        torch, ctx = self.torch, self.ctx
        F = sym.shape[0]
        out = torch.empty_like(sym)
        sw = torch.empty(F, dtype=torch.int32, device=self.dev)
        res = torch.empty(F, dtype=torch.int32, device=self.dev)
        st = torch.empty(F, dtype=torch.int32, device=self.dev)
        for _ in range(warmup):
            ctx.decode(h, sym, era, out=out, sweeps=sw, residual=res, status=st)
            ctx.synchronize()   # (untimed) the library sizes its ML schedule arena from the demand of the calls already finished
        if after_steps and warmup > 0 and self.world > 1:
            after_steps(out, sw, res, st)   # (untimed) the collective's first call sets up its communicator and loads its kernels
        ctx.get_profile()
        ctx.set_profiling(True)
        self.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.decode(h, sym, era, out=out, sweeps=sw, residual=res, status=st)
        extra = after_steps(out, sw, res, st) if after_steps else None
        self.barrier()
        dt = time.perf_counter() - t0
        ctx.set_profiling(False)
        prof = ctx.get_profile()
        if detail:   # break-down of the two-kernel kinds (tier 2 alone, solve kernel alone): two more steps OUTSIDE the timed region
            ctx.set_profiling(2)
            for _ in range(2):
                ctx.decode(h, sym, era, out=out, sweeps=sw, residual=res, status=st)
            ctx.set_profiling(False)
            p2 = ctx.get_profile()
            for kk in ("apply_tier2", "ml_solve"):
                prof[kk] = p2[kk]
        names = ctx.profile_kernel_names()
        return dict(dt=dt, out=out, sw=sw, res=res, st=st, extra=extra, names=names,
                    kernel_ms={kk: (v[0] / max(v[1], 1)) for kk, v in prof.items() if v[1] > 0})


def summarize(g, r, cw, n, k, S, steps, frames_all_ranks, checks=True):
    """Common numbers of one timed decode run (checks=False: the timing figures only, no statistics or verification)."""
    torch = g.torch
    F = cw.shape[0]
    ms = r["dt"] / steps * 1e3
    timing = {
        "frames": F, "frames_per_s": frames_all_ranks * steps / r["dt"], "ms_per_step": ms, "steps": steps,
        "recovered_GBps": frames_all_ranks * steps / r["dt"] * k * S / 1e9,
        "kernel_ms": r["kernel_ms"], "kernels": r["names"],
    }
    if not checks:
        return timing
    ok_frames = r["st"] <= 1
    verified = bool(torch.equal(r["out"][ok_frames], cw[ok_frames]))
    resid = r["res"][r["res"] > 0].float()
    ab = alg_bytes_per_frame(n, S) * F
    return {
        **timing,
        "alg_bytes_per_step": ab, "roofline_frac": ab / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
        "sweeps_hist": torch.bincount(r["sw"], minlength=12).cpu().numpy().tolist(),
        "ml_trigger_rate": float((r["res"] > 0).float().mean()) if F else 0.0,
        "rank_deficient_rate": float((r["st"] == 2).float().mean()) if F else 0.0,
        "undecoded_rate": float((r["st"] >= 2).float().mean()) if F else 0.0,
        "mean_residual": float(resid.mean()) if resid.numel() else 0.0,
        "max_residual": int(resid.max()) if resid.numel() else 0,
        "verified": verified,
    }


def pick_samples(r, sym, era, want_ml):
    """A few frames of the timed output for the oracle spot check (after the timed region): the first two, plus -- when the
    ML stage ran -- the first frame it solved and the first rank-deficient one."""
    ids = [0, 1]
    if want_ml:
        for code in (1, 2):
            hit = (r["st"] == code).nonzero().flatten()
            if hit.numel():
                ids.append(int(hit[0]))
    ids = sorted(set(i for i in ids if i < sym.shape[0]))
    take = lambda t: t[ids].cpu().numpy()   # noqa: E731
    return ids, take(sym), take(era), take(r["out"]), take(r["sw"]), take(r["st"])


def dump_outputs(path, r, rank, world):
    """--dump-outputs: what the timed decode returned in its last step, as float32 .npy files under `path` (each value a byte or
    a small count, exact in float32): `sweeps`, `residual` and `status` of every frame, and `decoded_sample`, a fixed seeded
    sample of the decoded symbols -- DUMP_FRAMES frames x all n symbols x DUMP_LANES byte lanes of the S-byte packets (the whole
    output is F x n x S bytes, 8.6 GB at the defaults).  With N > 1 every rank writes its own frames, `<name>_rank<r>.npy`."""
    import torch
    out = r["out"]
    F, n = out.shape[0], out.shape[1]
    S = out.shape[2] if out.ndim == 3 else 1
    rng = np.random.default_rng(DUMP_SEED)
    frames = np.sort(rng.choice(F, size=min(DUMP_FRAMES, F), replace=False))
    lanes = np.sort(rng.choice(S, size=min(DUMP_LANES, S), replace=False))
    fi = torch.from_numpy(frames).to(out.device)
    li = torch.from_numpy(lanes).to(out.device)
    arrays = {"decoded_sample": out.reshape(F, n, S).index_select(0, fi).index_select(2, li)}
    # the status words of every frame (12 B per frame as float32) while they fit in a quarter of the budget, else of the sampled frames
    all_frames = 12 * F <= DUMP_LIMIT_BYTES // 4
    for key, name in (("sw", "sweeps"), ("res", "residual"), ("st", "status")):
        arrays[name] = r[key] if all_frames else r[key].index_select(0, fi)
    arrays = {name: a.cpu().numpy().astype(np.float32) for name, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} bytes exceed {DUMP_LIMIT_BYTES}"
    os.makedirs(path, exist_ok=True)
    suffix = f"_rank{rank}" if world > 1 else ""
    for name, a in arrays.items():
        np.save(os.path.join(path, name + suffix + ".npy"), a)


def oracle_check(code_ind, S, sample):
    from ldpc_erasure_codes_amd import codes
    from oracle import oracle_py
    oc = oracle_py.OracleCode(codes.load_builtin(code_ind))
    ids, sym, era, out, sw, st = sample
    ok = True
    for i in range(len(ids)):
        if S == 1:
            o, osw, _, ost = oc.decode_batch_s1(sym[i:i + 1], era[i:i + 1])
            ok = ok and bool(np.array_equal(o[0], out[i])) and int(osw[0]) == int(sw[i]) and int(ost[0]) == int(st[i])
        else:
            o, _, it, info, _ = oc.decode_packets(sym[i], era[i])
            ok = ok and bool(np.array_equal(o, out[i])) and it == int(sw[i])
    return ok, len(ids)


def run_cfg2(g, args):
    """Headline.  Returns {S: result}."""
    torch = g.torch
    from ldpc_erasure_codes_amd import sharding
    h, n, k = g.code(1)
    F = args.frames
    result = {}
    for S in ([args.S, 1] if (args.full and args.S != 1 and not args.no_s1) else [args.S]):
        steps = args.steps if S == args.S else max(args.steps, 20)
        cw, sym, era, _ = g.make_batch("cfg2", 1, S, frame0=g.rank * F, nframes=F)   # every rank its own frames
        counts = [F] * g.world
        # the one collective of the job: final gather of the status words (12 B/frame) over RCCL/xGMI
        r = g.time_decode(h, sym, era, steps, args.warmup,
                          after_steps=lambda out, sw, res, st: sharding.gather_status(torch.stack([sw, res, st]), counts))
        r["dt"] = sharding.max_over_ranks(r["dt"], g.dev)
        assert len(r["extra"]) == g.world
        if S == args.S and args.dump_outputs:
            dump_outputs(args.dump_outputs, r, g.rank, g.world)
        if not args.full:   # a plain run: the headline's timing and nothing else
            result[S] = summarize(g, r, cw, n, k, S, steps, g.world * F, checks=False)
            del cw, sym, era, r
            continue
        s = summarize(g, r, cw, n, k, S, steps, g.world * F)
        s["verified"] = s["verified"] and int(r["st"].max()) == 0   # every frame of cfg 2 decodes to its codeword
        s["sample"] = pick_samples(r, sym, era, False)
        kind = "apply" if S > 1 else "peel"
        kavg = r["kernel_ms"][kind]  # ms per launch of the dominant kernel, HIP events on its own stream

        ab = alg_bytes_per_frame(n, S) * F
        ach = ab / (kavg * 1e-3) / 1e9 if kavg > 0 else 0.0
        copy_gbps = None
        if S >= 16:
            # the copy rate this box reaches (same buffers, same streaming loads/stores), quoted next to the
            # nominal HBM peak; bytes moved = read + write
            # best single launch over 20 repetitions of five launch shapes, at two sizes (the whole batch and a quarter of it)
            copy_gbps = 0.0
            for nb in (sym.numel(), (sym.numel() // 4) & ~4095):
                if nb >= 4096:
                    copy_ms = g.ctx.copy_probe(sym, r["out"], reps=20, nbytes=nb)
                    copy_gbps = max(copy_gbps, 2.0 * nb / (copy_ms * 1e-3) / 1e9)
        traffic, tsrc = pmc_traffic(r["names"][kind]) if F == 4096 else (None, None)
        s["roofline"] = {"bound": "hbm", "kernel": r["names"][kind], "achieved": ach, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": ach / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": tsrc,
                         "alg_bytes_per_launch": ab, "avg_launch_ms": kavg, "copy_kernel_GBps": copy_gbps,
                         "frac_of_copy": (ach / copy_gbps) if copy_gbps else None}
        s["sustained"] = None
        if S == args.S and args.sustain_seconds > 0:
            # the same step repeated for a few seconds of wall clock (the timed region above is K steps = tens of ms): a
            # sustained-clock figure, and something an outside GPU-busy sampler can see.  Reported next to `value`, never as it.
            out2, sw2, res2, st2 = r["out"], r["sw"], r["res"], r["st"]
            n_sus = max(steps, int(args.sustain_seconds / max(r["dt"] / steps, 1e-6)))
            g.barrier()
            t1 = time.perf_counter()
            for _ in range(n_sus):
                g.ctx.decode(h, sym, era, out=out2, sweeps=sw2, residual=res2, status=st2)
            g.barrier()
            dts = sharding.max_over_ranks(time.perf_counter() - t1, g.dev)
            s["sustained"] = {"steps": n_sus, "seconds": dts, "ms_per_step": dts / n_sus * 1e3, "frames_per_s": g.world * F * n_sus / dts,
                              "verified": bool(torch.equal(out2, cw))}
        s["pipelined"] = None
        if S == args.S and S > 1 and args.sustain_seconds > 0:
            # Not `value`: the same K steps dealt alternately to TWO contexts, each on its own stream -- independent batches pipeline
            # (the peel kernel of one batch runs beside the packet kernel of the other: tools/two_stream_probe.py).  A host that
            # decodes a stream of batches gets this rate; `value` stays the rate of one context, one batch after the other.
            from ldpc_erasure_codes_amd import api as _api, codes as _codes
            ctx2 = _api.Context(torch.cuda.current_device())
            h2 = ctx2.load_builtin_code(1, _codes.DEFAULT_COEF_SEED[1])
            outb = torch.empty_like(sym)
            swb, resb, stb = (torch.empty(F, dtype=torch.int32, device=g.dev) for _ in range(3))
            outa, swa, resa, sta = r["out"], r["sw"], r["res"], r["st"]

            def step(i):
                if i & 1:
                    ctx2.decode(h2, sym, era, out=outb, sweeps=swb, residual=resb, status=stb)
                else:
                    g.ctx.decode(h, sym, era, out=outa, sweeps=swa, residual=resa, status=sta)
            kp = max(steps, 20) & ~1
            for i in range(4):
                step(i)
            ctx2.synchronize()
            g.barrier()
            t2 = time.perf_counter()
            for i in range(kp):
                step(i)
            ctx2.synchronize()
            g.barrier()
            dtp = sharding.max_over_ranks(time.perf_counter() - t2, g.dev)
            s["pipelined"] = {"contexts": 2, "steps": kp, "ms_per_step": dtp / kp * 1e3, "frames_per_s": g.world * F * kp / dtp,
                              "verified": bool(torch.equal(outa, cw) and torch.equal(outb, cw)),
                              "note": "the K steps dealt alternately to two contexts on two streams (independent batches overlap); not `value`"}
            ctx2.close()
            del outb
        s["encoder"] = None
        if S == args.S and S > 1 and args.sustain_seconds > 0:
            # SURVEY 8(f) row 1, the step before the path: the systematic encoder on the same batch (k S bytes in, n S bytes out per frame)
            srcb = cw[:, :k, :].contiguous()
            enc = torch.empty_like(cw)
            g.ctx.encode(h, srcb, out=enc)
            g.barrier()
            t3 = time.perf_counter()
            for _ in range(5):
                g.ctx.encode(h, srcb, out=enc)
            g.barrier()
            dte = sharding.max_over_ranks(time.perf_counter() - t3, g.dev) / 5
            eb = float(F) * (k + n) * S
            s["encoder"] = {"ms_per_batch": dte * 1e3, "frames_per_s": g.world * F / dte, "alg_bytes_per_batch": eb,
                            "GBps": eb / dte / 1e9, "of_hbm_peak": eb / dte / 1e9 / HBM_PEAK_GBPS, "verified": bool(torch.equal(enc, cw))}
            del srcb, enc
        s["xgmi_probe"] = None
        if S == args.S and g.world > 1 and g.backend == "nccl":
            # not part of `value`: one RCCL all-gather of a 64 MB slice of the decoded output per rank, so that a multi-GPU run
            # of the default command also yields an xGMI figure (the job's own collective moves only 12 B per frame)
            nb = min(64 << 20, r["out"].numel())
            piece = r["out"].reshape(-1)[:nb]
            flat = torch.empty(g.world * nb, dtype=torch.uint8, device=g.dev)
            g.dist.all_gather_into_tensor(flat, piece)
            g.barrier()
            t1 = time.perf_counter()
            for _ in range(3):
                g.dist.all_gather_into_tensor(flat, piece)
            g.barrier()
            dtg = sharding.max_over_ranks((time.perf_counter() - t1) / 3, g.dev)
            s["xgmi_probe"] = {"collective": "all_gather_into_tensor", "bytes_per_rank": nb, "ms": dtg * 1e3,
                               "recv_GBps_per_rank": (g.world - 1) * nb / dtg / 1e9,
                               "verified": bool(torch.equal(flat[g.rank * nb:(g.rank + 1) * nb], piece))}
            del flat
        s["inplace"] = None
        if S >= 16 and g.world == 1:
            # extension, reported separately and never as `value`: LDPC_AMD_INPLACE decodes inside the caller's frame buffer
            # and writes only the erased symbols (the reference always returns a copy)
            buf = sym.clone()
            sw, res, st = r["sw"], r["res"], r["st"]
            for _ in range(2):
                g.ctx.decode(h, buf, era, sweeps=sw, residual=res, status=st, inplace=True)
            g.ctx.get_profile()
            g.ctx.set_profiling(True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(steps):
                g.ctx.decode(h, buf, era, sweeps=sw, residual=res, status=st, inplace=True)
            torch.cuda.synchronize()
            dti = time.perf_counter() - t1
            g.ctx.set_profiling(False)
            pi = g.ctx.get_profile()
            s["inplace"] = {"ms_per_step": dti / steps * 1e3, "frames_per_s": F * steps / dti, "verified": bool(torch.equal(buf, cw)),
                            "kernel_ms": {kk: (v[0] / max(v[1], 1)) for kk, v in pi.items()}}
            del buf
        result[S] = s
        del cw, sym, era, r
        torch.cuda.empty_cache()
    return result, n, k


def run_cfg3(g, args, S):
    torch = g.torch
    h, n, k = g.code(1)
    cw, sym, era, keep = g.make_batch("cfg3", 1, S, frame0=0, nframes=WORKLOADS["cfg3"]["frames"])
    steps = max(3, min(args.steps, 10))
    r = g.time_decode(h, sym, era, steps, min(args.warmup, 2), detail=True)
    s = summarize(g, r, cw, n, k, S, steps, cw.shape[0])
    s["workload"] = (f"S={S} bytes/symbol, BASELINE cfg3: (2040,1530) hybrid MP+ML, Gilbert-Elliott alpha={GE_PARAMS[0]} beta={GE_PARAMS[1]} "
                     f"bias={GE_PARAMS[2]:g} (chain carried across frames), {WORKLOADS['cfg3']['frames']} frames drawn, "
                     f"{cw.shape[0]} with E0 < n-k decoded (the rest skipped as in ErasureCodes_NonBinaryLDPCSim.m:216)")
    s["frames_skipped_E0_ge_m"] = int((~keep).sum())
    s["sample"] = pick_samples(r, sym, era, True)
    s["ml_stage_stats"] = g.ctx.ml_stats()   # of the last step: residual frames, through the fast path, flagged by its test, deferred
    if S > 1:
        # the ML stage's other modes on the same batch (ML_PI knob): 0 = exact elimination only (round 2's
        # path), 2 = fast path without the consistency test (for callers that know their symbols are codewords with erasures).
        # The line above is the default, 1: fast path + consistency test -- the reference's bytes on any input.
        s["ml_stage_mode"] = "ML_PI=1 (default): fast path with consistency test, exact elimination for what it leaves or flags"
        modes = {}
        for name, val in (("ML_PI=0 exact elimination only", "0"), ("ML_PI=2 fast path, no consistency test", "2")):
            g.ctx.configure("LDPC_AMD_ML_PI", val)
            rm = g.time_decode(h, sym, era, 4, 2)
            sm = summarize(g, rm, cw, n, k, S, 4, cw.shape[0])
            modes[name] = {"ms_per_step": sm["ms_per_step"], "roofline_frac": sm["roofline_frac"], "verified": sm["verified"],
                           "same_bytes_as_default": bool(torch.equal(rm["out"], r["out"]))}
            del rm
        g.ctx.configure("LDPC_AMD_ML_PI", None)
        s["ml_stage_other_modes"] = modes
    del cw, sym, era, r
    torch.cuda.empty_cache()
    return s


def run_cfg4(g, args):
    """(4080,3060) LDPC next to 16 x RS(255,223) over the same 4080-symbol erasure patterns (block i = symbols
    255 i ... 255 i + 254, ErasureCodes_NonBinaryLDPCSim.m:210-214), S = 1."""
    torch, ctx = g.torch, g.ctx
    from ldpc_erasure_codes_amd import codes
    if not codes.have_builtin(3):
        return None
    h, n, k = g.code(3)
    F = WORKLOADS["cfg4"]["frames"]
    cw, sym, era, _ = g.make_batch("cfg4", 3, 1, frame0=0, nframes=F)
    steps = 3
    r = g.time_decode(h, sym, era, steps, 1)
    s = summarize(g, r, cw, n, k, 1, steps, F)
    s["workload"] = ("S=1 byte/symbol, BASELINE cfg4: (4080,3060) GF(256) LDPC [matrix synthesised by tools/hgen.cpp -- the reference "
                     "names the code but does not ship it; column profile ACHIEVED, not the script's: source columns of degree 3-10 "
                     "(none of degree 12), parity columns mostly of degree 3, DESIGN.md section 8] vs 16 x RS(255,223) on the same erasure patterns, 65536 frames, uniform 10 %")
    s["sample"] = pick_samples(r, sym, era, False)
    rn, rk = WORKLOADS["cfg4"]["rs"]
    rs = ctx.rs_create(rn, rk)
    blocks = era.reshape(F * (n // rn), rn)
    received = blocks == 0
    can = received.sum(dim=1) >= rk                       # RS decode attempted only for blocks with >= k received
    order = torch.argsort((~received).to(torch.uint8), dim=1, stable=True)[:, :rk]   # first k received positions, ascending
    sel = torch.nonzero(can).flatten()
    B = int(sel.numel())
    rsrc = torch.empty((B, rk), dtype=torch.uint8, device=g.dev)
    ctx.synth_source(SEED_SRC + 77, 0, B, rk, 1, rsrc)
    rcw = ctx.rs_encode(rs, rn, rk, rsrc)
    idx = order[sel].to(torch.int16).contiguous()
    val = torch.gather(rcw, 1, order[sel]).contiguous()
    msg = ctx.rs_decode(rs, idx, val)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(steps):
        msg = ctx.rs_decode(rs, idx, val)
    ev1.record()
    torch.cuda.synchronize()
    trs = (time.perf_counter() - t0) / steps
    rs_ab = rs_alg_bytes_per_block(rk, 1) * B
    s_rs = {"blocks_total": F * (n // rn), "blocks_decodable": B, "blocks_per_s": B / trs, "ms_per_step": trs * 1e3,
            "kernel_ms": {"rs_decode": ev0.elapsed_time(ev1) / steps}, "frame_equivalents_per_s": B / (n // rn) / trs,
            "alg_bytes_per_step": rs_ab, "roofline_frac": rs_ab / trs / 1e9 / HBM_PEAK_GBPS,
            "verified": bool(torch.equal(msg, rsrc)),
            "block_failure_rate": 1.0 - B / float(F * (n // rn))}
    del cw, sym, era, r, rcw, idx, val, order, msg
    torch.cuda.empty_cache()
    return {"ldpc": s, "rs": s_rs}


def run_cfg4_packets(g, args, S=1024):
    """(4080,3060) on the packet (HBM-roofline) path -- north_star names this matrix next to (2040,1530) -- and RS(255,223)
    in packet mode (the paper's system model: S RS codecs in parallel, Latex/Milcom_2022_ErasureCodes.tex:53,125) on the
    erasure patterns of the same frames.  4096 frames (the first 4096 of cfg 4's stream): 65536 x 4080 x 1 KB does not fit."""
    torch, ctx = g.torch, g.ctx
    from ldpc_erasure_codes_amd import codes
    if not codes.have_builtin(3):
        return None
    h, n, k = g.code(3)
    F = WORKLOADS["cfg4p"]["frames"]
    cw, sym, era, _ = g.make_batch("cfg4p", 3, S, frame0=0, nframes=F)
    steps = max(3, min(args.steps, 10))
    r = g.time_decode(h, sym, era, steps, 2)
    s = summarize(g, r, cw, n, k, S, steps, F)
    s["workload"] = (f"S={S} bytes/symbol, BASELINE cfg4's code on the packet path: (4080,3060) GF(256) LDPC [matrix synthesised by "
                     f"tools/hgen.cpp -- the reference names the code but does not ship it; achieved column profile: degrees 3-10, none of degree 12, "
                     f"DESIGN.md section 8], uniform 10 %, {F} frames "
                     f"(= {2 * F * n * S / 1e9:.1f} GB in + out; 65536 frames x 1 KB packets would be 548 GB)")
    s["verified"] = s["verified"] and int(r["st"].max()) == 0
    kavg = r["kernel_ms"]["apply"]   # both tiers (tier 2 takes the handful of frames with more than tcap steps)
    ab = alg_bytes_per_frame(n, S) * F
    ach = ab / (kavg * 1e-3) / 1e9 if kavg > 0 else 0.0
    traffic, tsrc = pmc_traffic(r["names"]["apply"], "cfg4p")
    s["roofline"] = {"bound": "hbm", "kernel": r["names"]["apply"], "achieved": ach, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": ach / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": tsrc,
                     "alg_bytes_per_launch": ab, "avg_launch_ms": kavg}
    s["plan"] = ctx.last_plan()
    s["S"] = S
    s["sample"] = pick_samples(r, sym, era, False)
    del sym, r
    torch.cuda.empty_cache()
    # the (4080,3060) encoder on the same frames: k S bytes in, n S bytes out per frame
    srcb = cw[:, :k, :].contiguous()
    enc = torch.empty_like(cw)
    ctx.encode(h, srcb, out=enc)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    for _ in range(5):
        ctx.encode(h, srcb, out=enc)
    torch.cuda.synchronize()
    dte = (time.perf_counter() - t3) / 5
    eb = float(F) * (k + n) * S
    enc_leg = {"ms_per_batch": dte * 1e3, "frames_per_s": F / dte, "alg_bytes_per_batch": eb, "GBps": eb / dte / 1e9,
               "of_hbm_peak": eb / dte / 1e9 / HBM_PEAK_GBPS, "verified": bool(torch.equal(enc, cw))}
    del cw, srcb, enc
    torch.cuda.empty_cache()

    # ---- RS(255,223), S-byte packets, on the same erasure patterns (block i = symbols 255 i ... 255 i + 254)
    rn, rk = WORKLOADS["cfg4"]["rs"]
    rs = ctx.rs_create(rn, rk)
    blocks = era.reshape(F * (n // rn), rn)
    received = blocks == 0
    can = received.sum(dim=1) >= rk
    order = torch.argsort((~received).to(torch.uint8), dim=1, stable=True)[:, :rk]
    sel = torch.nonzero(can).flatten()
    B = int(sel.numel())
    rsrc = torch.empty((B, rk, S), dtype=torch.uint8, device=g.dev)
    ctx.synth_source(SEED_SRC + 78, 0, B, rk, S, rsrc)
    rcw = ctx.rs_encode(rs, rn, rk, rsrc)
    idx = order[sel].to(torch.int16).contiguous()
    val = rcw[torch.arange(B, device=g.dev)[:, None], order[sel]].contiguous()
    del rcw
    msg = ctx.rs_decode(rs, idx, val)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(steps):
        msg = ctx.rs_decode(rs, idx, val, out=msg)
    ev1.record()
    torch.cuda.synchronize()
    trs = (time.perf_counter() - t0) / steps
    kms = ev0.elapsed_time(ev1) / steps
    rs_ab = rs_alg_bytes_per_block(rk, S) * B
    missing = (order[sel] >= rk).sum(dim=1).float()   # received repair symbols among the first k = missing source symbols
    s_rs = {"workload": f"S={S} bytes/symbol, RS(255,223) erasure decode of the {B} decodable blocks (of {F * (n // rn)}: 16 per frame "
                        f"pattern, uniform 10 %), k*S in + 2k + k*S out = {rs_alg_bytes_per_block(rk, S)} algorithmic bytes per block",
            "blocks_total": F * (n // rn), "blocks_decodable": B, "blocks_per_s": B / trs, "ms_per_step": trs * 1e3,
            "kernel_ms": {"rs_decode": kms}, "frame_equivalents_per_s": B / (n // rn) / trs,
            "recovered_GBps": B / trs * rk * S / 1e9, "mean_missing_source_symbols": float(missing.mean()),
            "gf_macs_per_block_row": float((missing * rk).mean()),
            "alg_bytes_per_step": rs_ab, "roofline_frac": rs_ab / (kms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
            "verified": bool(torch.equal(msg, rsrc)), "block_failure_rate": 1.0 - B / float(F * (n // rn))}
    # oracle spot check of two blocks (after the timed region)
    s_rs["sample"] = (idx[:2].cpu().numpy().astype(np.uint16), val[:2].cpu().numpy(), msg[:2].cpu().numpy())
    del era, idx, val, order, msg, rsrc
    torch.cuda.empty_cache()
    return {"ldpc": s, "rs": s_rs, "encoder": enc_leg}


def run_cfg5(g, args, total, gather, S=1):
    """Mixed (4000,2000) + (2040,1530) stream, 1:1, sharded over the ranks: bucket by code, each rank decodes its block of
    every bucket, then ONE gather (status words, or outputs + status words).  Decode and gather are timed separately."""
    torch = g.torch
    from ldpc_erasure_codes_amd import sharding
    ids = sharding.mixed_stream_ids(total)
    handles = {ci: g.code(ci) for ci in WORKLOADS["cfg5"]["codes"]}
    mine = sharding.shard_mixed(ids, g.rank, g.world)
    batches = {}
    for ci, gidx in mine.items():
        cw, sym, era, keep = g.make_batch("cfg5", ci, S, frame_ids=gidx)
        assert bool(keep.all())
        F = sym.shape[0]
        batches[ci] = dict(cw=cw, sym=sym, era=era, out=torch.empty_like(sym),
                           sw=torch.empty(F, dtype=torch.int32, device=g.dev), res=torch.empty(F, dtype=torch.int32, device=g.dev),
                           st=torch.empty(F, dtype=torch.int32, device=g.dev))

    def decode_all():
        for ci, b in batches.items():
            g.ctx.decode(handles[ci][0], b["sym"], b["era"], out=b["out"], sweeps=b["sw"], residual=b["res"], status=b["st"])

    steps = max(3, min(args.steps, 10))

    def gather_all():
        shard = {ci: {"gidx": mine[ci], "out": b["out"], "words": torch.stack([b["sw"], b["res"], b["st"]])} for ci, b in batches.items()}
        return sharding.gather_mixed(ids, shard, g.world, gather)

    for _ in range(max(1, min(args.warmup, 2))):
        decode_all()
    full = gather_all()   # warm-up of the gather as well (its first call pays one-time allocations and, with N > 1, RCCL's set-up: 19 ms against 0.4)
    del full
    g.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        decode_all()
    g.barrier()
    t1 = time.perf_counter()
    full = gather_all()
    g.barrier()
    t2 = time.perf_counter()
    dt_dec = sharding.max_over_ranks(t1 - t0, g.dev)
    dt_gat = sharding.max_over_ranks(t2 - t1, g.dev)
    ok = all(bool(torch.equal(b["out"], b["cw"])) and int(b["st"].max()) == 0 for b in batches.values() if b["sym"].shape[0])
    gathered_frames = sum(int(v["words"].shape[1]) for v in full.values())
    gbytes = sum(int(v["words"].numel()) * 4 + (int(v["out"].numel()) if v["out"] is not None else 0) for v in full.values())
    ab = sum(alg_bytes_per_frame(handles[ci][1], S) * int((ids == ci).sum()) for ci in handles)
    per_step = (dt_dec / steps) + dt_gat          # one job = decode the stream once + the final gather
    s = {"workload": f"S={S} bytes/symbol, BASELINE cfg5: mixed (4000,2000) + (2040,1530) stream 1:1, uniform 10 %, {total} frames over "
                     f"{g.world} GPU(s) (bucketed by code, contiguous blocks per rank), final gather of {gather}",
         "S": S,
         "frames": total, "frames_this_rank": sum(b["sym"].shape[0] for b in batches.values()),
         "frames_per_s": total / per_step, "decode_ms_per_step": dt_dec / steps * 1e3, "gather_ms": dt_gat * 1e3,
         "gather": gather, "gathered_frames": gathered_frames, "gathered_bytes": gbytes, "gathered_bytes_per_rank": gbytes,
         "gather_GBps_per_rank": gbytes / dt_gat / 1e9 if dt_gat > 0 else None,
         "alg_bytes_per_step": ab, "roofline_frac": ab / (dt_dec / steps) / 1e9 / HBM_PEAK_GBPS / g.world,
         "steps": steps, "verified": ok and gathered_frames == total}
    b0 = batches[WORKLOADS["cfg5"]["codes"][0]]
    s["samples"] = {}
    for ci, b in batches.items():
        if b["sym"].shape[0] >= 2:
            r = dict(out=b["out"], sw=b["sw"], st=b["st"])
            s["samples"][ci] = pick_samples(r, b["sym"], b["era"], False)
    del b0
    return s


# ----------------------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4096, help="frames per GPU per step (BASELINE cfg 2: 4096)")
    ap.add_argument("--S", type=int, default=1024, help="bytes per symbol (1 = Matlab model, 1024 = FPGA packet)")
    ap.add_argument("--config", default="2", choices=["2", "3", "4", "5"],
                    help="2 (default): headline cfg 2 + the 'configs' block with cfg 3/4/5 at N = 1; 3/4/5: that config alone "
                         "(5 = the 65536-frame mixed stream sharded over --gpus ranks)")
    ap.add_argument("--gather", default="status", choices=["status", "outputs"], help="cfg 5: what the final gather moves")
    ap.add_argument("--total-frames", type=int, default=None, help="cfg 5: frames of the whole stream (default 65536)")
    ap.add_argument("--cfg5-S", type=int, default=1, help="cfg 5 alone (--config 5): bytes per symbol (e.g. 64 with --gather outputs)")
    ap.add_argument("--cpu-seconds", type=float, default=3.0, help="CPU-baseline decode time per worker and leg")
    ap.add_argument("--sustain-seconds", type=float, default=5.0,
                    help="after the timed K steps, repeat the headline step for about this long and report it as `sustained` (0: off)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-configs", action="store_true", help="headline only (skip the cfg 3/4/5 block)")
    ap.add_argument("--no-s1", action="store_true", help="skip the S = 1 companion runs (profiling of one batch shape)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: S = 1 companion, CPU baselines, the cfg 3/4/5 block or --config 3/4/5, sustained / "
                         "pipelined / encoder / in-place / copy-probe figures, PMC roofline, oracle spot checks, detail file")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed headline step's outputs to DIR/<name>.npy (float32; a fixed sample of the symbols)")
    ap.add_argument("--detail-out", default=os.path.join(ROOT, "bench_detail.json"),
                    help="--full: file for the whole result (the line on stdout is the compact form)")
    args = ap.parse_args()
    if args.config != "2" and not args.full:
        ap.error(f"--config {args.config} is a side configuration: run it with --full")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with torch.distributed.run", file=sys.stderr)
        sys.exit(2)
    want_block = args.full and args.config == "2" and world == 1 and not args.no_configs
    do_cpu = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline

    # ---- CPU legs first (forked workers must not inherit a HIP context)
    cpu = {}
    if do_cpu:
        T = args.cpu_seconds
        if args.config == "2":
            cpu[("cfg2", args.S)] = cpu_baseline("cfg2", args.S, T)
            if args.S != 1:
                cpu[("cfg2", 1)] = cpu_baseline("cfg2", 1, T)
            cpu["cfg1"] = cpu_cfg1()
        def side_leg(cfg, S_):   # a failing side config must not cost the headline line: it is reported, not raised
            try:
                cpu[(cfg, S_)] = cpu_baseline(cfg, S_, T)
            except Exception as e:   # noqa: BLE001
                if not want_block:
                    raise
                print(f"bench.py: CPU baseline of {cfg} S={S_} failed: {e!r}", file=sys.stderr)
        if want_block or args.config == "3":
            for S_ in sorted({1024, 1} if want_block else ({args.S} if args.no_s1 else {args.S, 1}), reverse=True):
                side_leg("cfg3", S_)
        if want_block or args.config == "4":
            side_leg("cfg4", 1)
            side_leg("cfg4p", 1024)
        if want_block or args.config == "5":
            side_leg("cfg5", 1)

    g = Gpu(args, rank, world, local_rank)
    line = None
    checks = []   # (where, code_ind, S, sample) -> oracle spot checks after the timed regions
    if args.config == "2":
        result, n, k = run_cfg2(g, args)
        block = {}
        if want_block:
            def side(name, fn):   # the side configs ride along: an exception there is reported in the block, the headline stays
                try:
                    r = fn()
                    if r:
                        block[name] = r
                except Exception as e:   # noqa: BLE001
                    import traceback
                    traceback.print_exc()
                    block[name + "_error"] = repr(e)
            for S in (1024, 1):
                side(f"cfg3_S{S}", lambda S=S: run_cfg3(g, args, S))
            side("cfg4", lambda: run_cfg4(g, args))
            side("cfg4_S1024", lambda: run_cfg4_packets(g, args))
            # the WHOLE 65536-frame stream on one GPU (the N = 1 anchor of the strong-scaling job) and one GPU's 1/8 share
            side("cfg5", lambda: run_cfg5(g, args, WORKLOADS["cfg5"]["frames"], args.gather))
            side("cfg5_one_eighth", lambda: run_cfg5(g, args, WORKLOADS["cfg5"]["frames"] // 8, args.gather))
            if "cfg5" in block:
                block["cfg5"]["workload"] += " -- the whole stream on ONE GPU: the N = 1 anchor of `--config 5 --gpus N` (strong scaling)"
            if "cfg5_one_eighth" in block:
                block["cfg5_one_eighth"]["workload"] += " -- ONE GPU's share (1/8) of the 8-GPU job"
            side("cfg5_S64_outputs", lambda: run_cfg5(g, args, 8192, "outputs", S=64))
    elif args.config == "3":
        block = {f"cfg3_S{S}": run_cfg3(g, args, S) for S in sorted({args.S} if args.no_s1 else {args.S, 1}, reverse=True)}
    elif args.config == "4":
        block = {"cfg4": run_cfg4(g, args)} if args.S == 1 else {"cfg4_S1024": run_cfg4_packets(g, args, args.S)}
    else:
        block = {"cfg5": run_cfg5(g, args, args.total_frames or WORKLOADS["cfg5"]["frames"], args.gather, S=args.cfg5_S)}
    non_default_knobs = g.ctx.knobs()   # (LDPC_AMD_* variables of the environment this process started under; '' = the shipped defaults)
    g.close()
    if rank != 0:
        return

    # ---- oracle spot checks of what was just timed (after the timed regions)
    def check(entry, code_ind, S):
        if entry is None or "sample" not in entry:
            return
        ok, cnt = oracle_check(code_ind, S, entry.pop("sample"))
        entry["verified"] = bool(entry["verified"] and ok)
        entry["oracle_spot_check_frames"] = cnt

    if args.config == "2":
        for S, r in result.items():
            check(r, 1, S)
    for name, e in block.items():
        if name.endswith("_error"):
            continue
        if name.startswith("cfg3"):
            check(e, 1, int(name.split("_S")[1]))
            key = ("cfg3", int(name.split("_S")[1]))
        elif name == "cfg4" and e:
            check(e["ldpc"], 3, 1)
            key = ("cfg4", 1)
        elif name == "cfg4_S1024" and e:
            check(e["ldpc"], 3, e["ldpc"]["S"])
            from oracle import oracle_py
            rn, rk = WORKLOADS["cfg4"]["rs"]
            rs_g = oracle_py.rs_generator(rn, rk)
            ix, vv, mm = e["rs"].pop("sample")
            ok = True
            for b in range(ix.shape[0]):
                for lane in (0, vv.shape[2] // 2, vv.shape[2] - 1):   # three byte lanes of the packet, each an S = 1 decode
                    om, _ = oracle_py.rs_decode(rs_g, ix[b], np.ascontiguousarray(vv[b, :, lane]))
                    ok = ok and bool(np.array_equal(om, mm[b, :, lane]))
            e["rs"]["verified"] = bool(e["rs"]["verified"] and ok)
            e["rs"]["oracle_spot_check_blocks"] = int(ix.shape[0])
            key = ("cfg4p", 1024)
        elif name.startswith("cfg5"):
            for ci, smp in e.pop("samples").items():
                ok, cnt = oracle_check(ci, e.get("S", 1), smp)
                e["verified"] = bool(e["verified"] and ok)
            key = ("cfg5", 1) if e.get("S", 1) == 1 else None
        else:
            continue
        if key in cpu:
            cb = cpu[key]
            tgt = e["ldpc"] if name in ("cfg4", "cfg4_S1024") else e
            tgt["cpu_baseline"] = cb
            if not name.startswith("cfg5") or world == 1:
                tgt["gpu_over_cpu_all_cores"] = tgt["frames_per_s"] / cb["value"] if cb.get("value") else None
            if name == "cfg4" and cb.get("rs_blocks_per_s"):
                e["rs"]["gpu_over_cpu_all_cores"] = e["rs"]["blocks_per_s"] / cb["rs_blocks_per_s"]

    if args.config == "2":
        main_r = result[args.S]
        line = {
            "metric": "decoded frames/sec (+ recovered GB/s), n=2040 k=1530 GF(256) LDPC hybrid MP+ML erasure decode "
                      "(cfg 2: MP path, ML stage armed but not triggered at 10 % erasures; cfg 3 in 'configs' exercises it)",
            "value": main_r["frames_per_s"], "unit": "frames/s", "recovered_GBps": main_r["recovered_GBps"],
            "n_gpus": world, "steps": main_r["steps"], "warmup": args.warmup, "ms_per_step": main_r["ms_per_step"],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": f"S={args.S} bytes/symbol, BASELINE cfg2: n=2040,k=1530 GF(256) LDPC (H_nb seed {2040}), 10% uniform "
                                   f"random erasures, batch={args.frames} frames per GPU, max_sweeps=10, ML on",
                       "frames_per_gpu": args.frames, "S": args.S, "per": 0.10, "code": "n2040_k1530",
                       "sharding": f"{world} x {args.frames} independent frames, status gather over RCCL"},
            "kernel_ms": main_r["kernel_ms"],
        }
        if args.full:
            line.update({"verified_bit_exact": main_r["verified"], "sweeps_hist": main_r["sweeps_hist"],
                         "ml_trigger_rate": main_r["ml_trigger_rate"], "roofline": main_r["roofline"]})
        if main_r.get("sustained"):
            line["sustained"] = main_r["sustained"]
        if main_r.get("pipelined"):
            line["pipelined_two_contexts"] = main_r["pipelined"]
        if main_r.get("encoder"):
            line["encoder"] = main_r["encoder"]
        if main_r.get("xgmi_probe"):
            line["xgmi_allgather_probe"] = main_r["xgmi_probe"]
        if main_r.get("inplace"):
            ip = main_r["inplace"]
            ach_ip = alg_bytes_per_frame(n, args.S) * args.frames / (ip["kernel_ms"]["apply"] * 1e-3) / 1e9
            line["inplace_extension"] = {
                "note": "LDPC_AMD_INPLACE (out == sym, only erased symbols written; the reference always returns a copy). Reported "
                        "against the same algorithmic bytes as SURVEY.md 8(d) prescribes; not the headline value.",
                "frames_per_s": ip["frames_per_s"], "ms_per_step": ip["ms_per_step"], "verified_bit_exact": ip["verified"],
                "kernel_ms": ip["kernel_ms"], "roofline_frac_vs_algorithmic_bytes": ach_ip / HBM_PEAK_GBPS}
        if ("cfg2", args.S) in cpu:
            line["cpu_baseline"] = cpu[("cfg2", args.S)]
            line["gpu_over_cpu"] = main_r["frames_per_s"] / cpu[("cfg2", args.S)]["value"]
        if "cfg1" in cpu:
            line["cfg1_cpu_reference_row"] = cpu["cfg1"]
        if 1 in result and args.S != 1:
            s1 = result[1]
            line["s1"] = {"note": "same batch with S=1 (one GF(256) element per symbol: the Matlab model, bit-exact incl. iterations); "
                                  "latency/LDS-bound by construction, HBM fraction reported for completeness",
                          "value": s1["frames_per_s"], "unit": "frames/s", "ms_per_step": s1["ms_per_step"], "steps": s1["steps"],
                          "verified_bit_exact": s1["verified"], "roofline": s1["roofline"]}
            if ("cfg2", 1) in cpu:
                line["s1"]["cpu_baseline"] = cpu[("cfg2", 1)]
                line["s1"]["gpu_over_cpu"] = s1["frames_per_s"] / cpu[("cfg2", 1)]["value"]
        if block:
            line["configs"] = block
    else:
        first = next(iter(block.values()))
        head = first["ldpc"] if args.config == "4" else first
        line = {
            "metric": f"decoded frames/sec, BASELINE cfg{args.config}", "value": head["frames_per_s"], "unit": "frames/s",
            "n_gpus": world, "steps": head["steps"], "warmup": args.warmup,
            "ms_per_step": head.get("ms_per_step", head.get("decode_ms_per_step")), "higher_is_better": True,
            "scaling": "strong" if args.config == "5" else "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": head["workload"]}, "verified_bit_exact": head["verified"], "configs": block,
        }
        if head.get("cpu_baseline"):
            line["cpu_baseline"] = head["cpu_baseline"]
    # ---- ONE line on stdout, short enough for the driver's tail: the required keys, `roofline`, `cpu_baseline`
    # and a flat per-config `summary` LAST; everything else (per-kernel name maps, workload prose, histograms, the ML stage's other
    # modes, the CPU legs' sample texts) goes to the detail file written by a --full run (--detail-out; not a committed file:
    # copy it under profiles/ deliberately when a line is recorded).
    line["non_default_knobs"] = non_default_knobs
    written = None
    if args.full:
        dpath = os.path.abspath(args.detail_out)
        try:
            with open(dpath, "w") as fh:
                json.dump(line, fh, indent=1)
            written = os.path.relpath(dpath, ROOT)
        except OSError as e:
            print(f"bench.py: could not write {dpath}: {e}", file=sys.stderr)
    print(json.dumps(compact_line(line, written), separators=(",", ":")))


def _r(x, sig=4):
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    try:
        return float(f"{float(x):.{sig}g}")
    except (TypeError, ValueError):
        return x


SHORT_KERNEL = (("ldpc_scatter_big_kernel", "scatter_big"), ("ldpc_scatter_kernel", "scatter"), ("ldpc_peel_kernel", "peel"),
                ("ldpc_ml_solve_kernel", "ml_solve"), ("ldpc_ml_kernel", "ml"), ("rs_decode_packets_kernel", "rs_packets"),
                ("rs_decode_s1_kernel", "rs_s1"))


def _short(name):
    if not name:
        return name
    for long, short in SHORT_KERNEL:
        if name.startswith(long):
            return short + name[len(long):].replace(" ", "")
    return name.replace(" ", "")


def _cfg_summary(e):
    """Flat per-config record: ms per step, frames/s, roofline fraction, dominant kernel + its ms, verified, ML stage."""
    if not e:
        return None
    o = {"ms": _r(e.get("ms_per_step", e.get("decode_ms_per_step"))), "fps": _r(e.get("frames_per_s", e.get("blocks_per_s"))),
         "frac": _r(e.get("roofline_frac"), 3), "ok": e.get("verified")}
    km = e.get("kernel_ms") or {}
    if km:
        dom = max(km, key=lambda kk: km[kk])
        o["k"] = _short((e.get("kernels") or {}).get(dom)) or dom
        o["kms"] = {kk: _r(v, 3) for kk, v in km.items() if v >= 0.02}
    if e.get("roofline"):
        o["kfrac"] = _r(e["roofline"]["frac"], 3)
    if e.get("ml_trigger_rate"):
        o["ml_rate"] = _r(e["ml_trigger_rate"], 3)
        o["rankdef"] = _r(e.get("rank_deficient_rate"), 2)
    if e.get("ml_stage_stats"):
        st = e["ml_stage_stats"]
        o["ml"] = [st["residual_frames"], st["fast_path_frames"], st["flagged_frames"], st["deferred_frames"]]
    if e.get("gather_ms") is not None:
        o["gather_ms"] = _r(e["gather_ms"], 3)
    cb = e.get("cpu_baseline")
    if cb:
        o["cpu"] = [_r(cb.get("single_thread"), 3), _r(cb.get("value"), 3)]
    return o


def compact_line(line, detail_file):
    keep = ("metric", "value", "unit", "recovered_GBps", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "verified_bit_exact", "ml_trigger_rate")
    out = {kk: line[kk] for kk in keep if kk in line}
    out["metric"] = out["metric"].split(" (cfg 2:")[0]
    out["value"] = _r(out["value"], 7)
    out["ms_per_step"] = _r(out["ms_per_step"], 5)
    if "recovered_GBps" in out:
        out["recovered_GBps"] = _r(out["recovered_GBps"], 5)
    if isinstance(out.get("config"), dict) and "workload" in out["config"]:
        out["config"] = dict(out["config"], workload=out["config"]["workload"][:160])
    if line.get("kernel_ms"):
        out["kernel_ms"] = {kk: _r(v, 4) for kk, v in line["kernel_ms"].items()}
    if line.get("roofline"):
        rf = line["roofline"]
        out["roofline"] = {kk: (_r(rf[kk], 5) if kk not in ("kernel", "bound", "unit", "traffic_source") else rf[kk]) for kk in
                           ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "alg_bytes_per_launch",
                            "avg_launch_ms", "copy_kernel_GBps", "frac_of_copy") if kk in rf}
        if out["roofline"].get("traffic_source"):
            out["roofline"]["traffic_source"] = out["roofline"]["traffic_source"].split(" (")[0] + " (replayed)"
    if line.get("cpu_baseline"):
        cb = line["cpu_baseline"]
        out["cpu_baseline"] = {"value": _r(cb.get("value"), 5), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
                               "sample": (cb.get("sample") or "")[:150], "single_thread": _r(cb.get("single_thread"), 4),
                               "cpu_model": cb.get("cpu_model")}
        out["gpu_over_cpu"] = _r(line.get("gpu_over_cpu"), 4)
    if detail_file:   # (written by --full runs only)
        out["detail_file"] = detail_file
    if line.get("non_default_knobs"):
        out["non_default_knobs"] = line["non_default_knobs"]   # a measurement under LDPC_AMD_* variables says so in the line
    sm = {}
    cfgs = line.get("configs") or {}
    for name in ("sustained", "pipelined_two_contexts"):
        if line.get(name):
            sm[name] = {"ms": _r(line[name]["ms_per_step"]), "fps": _r(line[name]["frames_per_s"]), "ok": line[name].get("verified")}
    if line.get("inplace_extension"):
        ip = line["inplace_extension"]
        sm["inplace"] = {"ms": _r(ip["ms_per_step"]), "fps": _r(ip["frames_per_s"]), "ok": ip["verified_bit_exact"]}
    for name in ("cfg5_S64_outputs", "cfg5_one_eighth", "cfg5"):
        if cfgs.get(name):
            sm[name] = _cfg_summary(cfgs[name])
    for name in ("cfg4", "cfg4_S1024"):
        if cfgs.get(name):
            sm[name + "_rs"] = _cfg_summary(cfgs[name].get("rs"))
            sm[name + "_ldpc"] = _cfg_summary(cfgs[name].get("ldpc"))
    for name, e in sorted(cfgs.items()):
        if name.endswith("_error"):
            sm[name] = str(e)[:120]
    if line.get("encoder"):
        en = line["encoder"]
        sm["encoder_2040"] = {"ms": _r(en["ms_per_batch"]), "frac": _r(en["of_hbm_peak"], 3), "ok": en["verified"]}
    if (cfgs.get("cfg4_S1024") or {}).get("encoder"):
        en = cfgs["cfg4_S1024"]["encoder"]
        sm["encoder_4080"] = {"ms": _r(en["ms_per_batch"]), "frac": _r(en["of_hbm_peak"], 3), "ok": en["verified"]}
    if line.get("s1"):
        s1 = line["s1"]
        sm["cfg2_S1"] = {"ms": _r(s1["ms_per_step"]), "fps": _r(s1["value"]), "frac": _r(s1["roofline"]["frac"], 3),
                         "ok": s1["verified_bit_exact"]}
        if s1.get("cpu_baseline"):
            sm["cfg2_S1"]["cpu"] = [_r(s1["cpu_baseline"].get("single_thread"), 3), _r(s1["cpu_baseline"].get("value"), 3)]
    for name in ("cfg3_S1", "cfg3_S1024"):     # the hybrid-ML config LAST: it must survive any tail cut
        if cfgs.get(name):
            sm[name] = _cfg_summary(cfgs[name])
    if sm:
        out["summary"] = sm
    return out


if __name__ == "__main__":
    main()
