"""GPU tests of the packet paths at the edges of their 32-bit address range ("Address range").

The hot kernels address a frame with a uniform 64-bit base and 32-bit per-lane offsets (24-bit multiplies) and rely on host-side
limits to stay correct: n * S < 2^32, S < 2^24, n < 2^16 for the scatter kernels (plan_scatter; beyond them the gather kernel runs),
n * (8 + S) < 2^32 and 8 + S < 2^24 for the packet-output encoder and stride * (8 + S) < 2^32 for its multi-flow form (beyond them
the composed senders), S < 2^23 for the streaming RS decode from frames (beyond it the generic kernel).  Here offsets have bit 31 set, frame bases lie beyond 2^32, and every fall-back
at a limit is taken -- on both sides of each limit, with sizes computed by tools/address_range.py, not written down.

Expected values: the CPU oracle at P = 4080 byte lanes (tests/address_range_cases.py), tiled.  All arithmetic is columnwise over
GF(256), so the big input is small[..., s mod P] and the big output must be the small output tiled alike
(tests/test_address_range_cpu.py shows that on the oracle alone); on the batch axis frame f is frame f mod 7 of a small batch.  No
power of two is a multiple of 4080: a displaced access reads or writes different content.  Everything large stays on the device;
outputs are pre-filled with a poison byte; every input and output lies between 4 KiB sentinel bands that are checked afterwards;
every byte is compared (tile groups on the device) and the sweeps, residual and status words of every frame; every case asserts
which kernel family ran.  Each case states its device memory need (below 24 GiB) and may skip only when less than that is free."""
import time

import numpy as np
import pytest

import address_range_cases as cases
from address_range_cases import ar
from ldpc_erasure_codes_amd import api, codes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_word_symbols import Arena  # noqa: E402  (4 KiB sentinel bands around every buffer)

POISON = 0xEE
GIB = 1 << 30
BUDGET = 24 * GIB
TIMES = {}


# ------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture
def ctx():
    """A context per case: its scratch (gigabytes at these sizes) goes with it."""
    torch.cuda.empty_cache()
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    torch.cuda.synchronize()
    c.close()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    TIMES[request.node.name] = time.perf_counter() - t0
    print(f"\n[address-range] {request.node.name}: {TIMES[request.node.name]:.2f} s")


def need(nbytes, what):
    """States the device footprint of a case; skips only when the device has less than that free."""
    assert nbytes < BUDGET, (what, nbytes)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    print(f"\n[address-range] {what}: needs {nbytes / GIB:.2f} GiB, {free / GIB:.1f} GiB free")
    if free < nbytes:
        pytest.skip(f"{what}: needs {nbytes / GIB:.1f} GiB of device memory, {free / GIB:.1f} GiB free")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a copy: the shared small problems are read-only)


def handle(ctx, which):
    code, _ = cases.get_code(which)
    if isinstance(which, int):
        return ctx.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which]), code
    return ctx.register_code(code), code


def tiled(arn, small, S):
    """A guarded device tensor [..., S]: the lane tiling of the small array."""
    return ar.fill_lanes(arn.new(tuple(small.shape[:-1]) + (S,)), dev(small))


def poisoned(arn, shape, dtype=torch.uint8):
    t = arn.new(shape, dtype)
    t.view(-1).view(torch.uint8).fill_(POISON)
    return t


def apply_name(ctx):
    return ctx.profile_kernel_names()["apply"]


class knobs:
    def __init__(self, ctx, kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.configure(k, v)

    def __exit__(self, *a):
        for k in self.kv:
            self.ctx.configure(k, None)
        assert self.ctx.knobs() == ""


def words_equal(got, want, tag):
    for name, a, b in zip(("sweeps", "residual", "status"), got, want):
        a = a.cpu().numpy()
        assert np.array_equal(a, b), f"{tag}: {name} {a.tolist()[:16]} != {b.tolist()[:16]}"


def run_decode(ctx, h, arn, sym, er, outs, small_want, family, tag, do_ml=1):
    """One decode into re-poisoned outputs; family, sentinels, every byte, every word."""
    out, sw, res, st = outs
    for t in outs:
        t.view(-1).view(torch.uint8).fill_(POISON)
    ctx.decode(h, sym, er, do_ml=do_ml, out=out, sweeps=sw, residual=res, status=st)
    arn.check()
    name = apply_name(ctx)
    print(f"[address-range] {tag}: {name}")
    assert name.startswith(family), f"{tag}: {name} ran, not {family}"
    bad = ar.lanes_mismatch(out, small_want[0])
    assert bad is None, f"{tag}: out differs from the tiled oracle result at (frame, row, tile, lane) {bad}"
    words_equal((sw, res, st), small_want[1:], tag)


def decode_outputs(arn, F, n, S):
    return (arn.new((F, n, S)),) + tuple(arn.new((F,), torch.int32) for _ in range(3))


def decode_case(ctx, which, S, variants, unit=16, frames=(0, 1)):
    """Decode from rows, F = 2 (frame 1 a non-codeword), once per (knobs, kernel family) of `variants`."""
    c = cases.light_case(which)
    c = {key: (v[list(frames)] if key != "want" else tuple(w[list(frames)] for w in v)) for key, v in c.items() if key != "code"}
    h, code = handle(ctx, which)
    if unit != 16:
        ctx.set_symbol_unit(unit)
    n, F = code.n, len(frames)
    need(2 * F * n * S + F * (code.m + 2) * (S + 16) + GIB, f"decode ({n},{code.k}) F={F} S={S}")
    arn = Arena()
    sym, er = tiled(arn, c["sym"], S), arn.new(c["era"].shape, src=c["era"])
    outs = decode_outputs(arn, F, n, S)
    want = (dev(c["want"][0]),) + c["want"][1:]
    for kv, family in variants:
        with knobs(ctx, kv):
            run_decode(ctx, h, arn, sym, er, outs, want, family, f"decode S={S} {kv}")
    assert ar.lanes_mismatch(sym, dev(c["sym"])) is None, "an out-of-place decode wrote to its input"


def encode_case(ctx, which, S, variants, unit=16, frames=(0, 1)):
    c = cases.light_case(which)
    c = {key: v[list(frames)] for key, v in c.items() if key in ("src", "cw")}
    h, code = handle(ctx, which)
    if unit != 16:
        ctx.set_symbol_unit(unit)
    n, k, F = code.n, code.k, len(frames)
    need(F * (n + k) * S + GIB, f"encode ({n},{k}) F={F} S={S}")
    arn = Arena()
    src = tiled(arn, c["src"], S)
    out = arn.new((F, n, S))
    want = dev(c["cw"])
    for kv, family in variants:
        with knobs(ctx, kv):
            out.fill_(POISON)
            ctx.encode(h, src, out=out)
            arn.check()
            name = ctx.encode_kernel_name()
        print(f"[address-range] encode S={S} {kv}: {name!r}")
        assert name.startswith(family), f"{name} ran, not {family}"
        bad = ar.lanes_mismatch(out, want)
        assert bad is None, f"encode S={S} {kv}: codeword differs at (frame, row, tile, lane) {bad}"
    assert ar.lanes_mismatch(src, dev(c["src"])) is None


SCATTER, GATHER, GATHER_W = "ldpc_scatter_kernel", "ldpc_apply_kernel", "ldpc_apply_words_kernel"
STATIC, STATIC_PKT = "ldpc_scatter_static_kernel", "ldpc_scatter_static_pkt_kernel"
DEC_VARIANTS = (({}, SCATTER), ({"SCATTER_TIERS": "1"}, SCATTER), ({"SCATTER_NT": "0"}, SCATTER), ({"ENC_PERSIST": "0"}, SCATTER),
                ({"APPLY": "gather"}, GATHER))
ENC_VARIANTS = (({}, STATIC), ({"SCATTER_TIERS": "1"}, STATIC), ({"SCATTER_NT": "0"}, STATIC), ({"ENC_PERSIST": "0"}, SCATTER),
                ({"APPLY": "gather"}, GATHER))


# ------------------------------------------------------------------------------------------------ A. n * S across 2^31
A_SIZES = ar.edge_pair(ar.LIM_SIGN, 300)
A_WORDS = ar.word_size_above(ar.LIM_SIGN, 300)


@pytest.mark.parametrize("S", A_SIZES)
def test_a_decode_across_bit_31(ctx, S):
    decode_case(ctx, "r300", S, DEC_VARIANTS)


def test_a_decode_words_above_bit_31(ctx):
    variants = tuple((kv, GATHER_W if fam == GATHER else fam) for kv, fam in DEC_VARIANTS)
    decode_case(ctx, "r300", A_WORDS, variants, unit=4)


@pytest.mark.parametrize("S", A_SIZES)
def test_a_encode_across_bit_31(ctx, S):
    encode_case(ctx, "r300", S, ENC_VARIANTS)


def test_a_encode_words_above_bit_31(ctx):
    encode_case(ctx, "r300", A_WORDS, tuple((kv, GATHER_W if fam == GATHER else fam) for kv, fam in ENC_VARIANTS), unit=4)


# ------------------------------------------------------------------------------------------------ B. (2040,1530) above 2^31, F = 3
B_S = ar.first_from(ar.LIM_SIGN, 2040)


@pytest.mark.parametrize("run", range(len(cases.B_RUNS)))
def test_b_2040_1530_every_status_class(ctx, run):
    """F = 3 frames of n * S > 2^31 bytes: frame 1 starts beyond 2^32.  Tier 2, the fast path's schedules, the solve kernel and
    the exact ML kernel all work on offsets with bit 31 set."""
    frames, do_ml = cases.B_RUNS[run]
    c = cases.b_case()
    sym_s, era, want_s = cases.b_run(c, frames, do_ml)
    h, code = handle(ctx, cases.B_CODE)
    n, F, S = code.n, 3, B_S
    assert n * S >= ar.LIM_SIGN and n * S < ar.LIM_OFFSET and 2 * n * S >= ar.LIM_OFFSET
    need(2 * F * n * S + F * (code.m + 2) * (S + 16) + 2 * GIB, f"decode (2040,1530) F={F} S={S} {frames}")
    arn = Arena()
    sym, er = tiled(arn, sym_s, S), arn.new(era.shape, src=era)
    outs = decode_outputs(arn, F, n, S)
    want = (dev(want_s[0]),) + want_s[1:]
    run_decode(ctx, h, arn, sym, er, outs, want, SCATTER, f"B {frames} do_ml={do_ml}", do_ml=do_ml)
    plan, names = ctx.last_plan(), ctx.profile_kernel_names()
    steps = era.sum(1).astype(np.int64) - want_s[2]
    print("[address-range] plan", plan, "steps", steps.tolist(), "status", want_s[3].tolist(), names)
    assert plan["two_tiers"] == 1 and plan["packet_bytes_per_workgroup"] == 256
    assert int(steps.min()) <= plan["tier1_cap"] < int(steps.max())
    assert names["apply_tier2"].startswith("ldpc_scatter_big_kernel")
    if do_ml:
        ms = ctx.ml_stats()
        print("[address-range] ml", ms)
        st = want_s[3]
        assert ms["residual_frames"] == int((st != 0).sum())
        assert names["ml_solve"].startswith("ldpc_ml_solve_kernel") and names["ml"] == "ldpc_ml_kernel"
        if "nc" in frames:
            assert ms["flagged_frames"] <= 1                      # the non-codeword: redone by the exact kernel where its system is inconsistent
        else:
            assert ms["fast_path_frames"] == int((st == 1).sum()) and ms["flagged_frames"] == 0
    assert ar.lanes_mismatch(sym, dev(sym_s)) is None


# ------------------------------------------------------------------------------------------------ C. the limits themselves
C_OFFSET = ar.edge_pair(ar.LIM_OFFSET, 300)          # n * S on either side of 2^32; both below 2^24
C_MUL24 = ar.edge_pair(ar.LIM_MUL24)                 # S on either side of 2^24; 64 * S far below 2^32
C_LIMITS = [("r300", C_OFFSET[0], True), ("r300", C_OFFSET[1], False), ("r64", C_MUL24[0], True), ("r64", C_MUL24[1], False)]
C_IDS = [f"{w}-{S}-{'scatter' if sc else 'gather'}" for w, S, sc in C_LIMITS]


@pytest.mark.parametrize("which,S,scatter", C_LIMITS, ids=C_IDS)
def test_c_decode_at_the_limit(ctx, which, S, scatter):
    n = cases.get_code(which)[0].n
    assert (n * S < ar.LIM_OFFSET and S < ar.LIM_MUL24) == scatter
    # (300,200): one frame is the whole range (4 GiB in, 4 GiB out) -- the non-codeword; (64,44): both frames
    decode_case(ctx, which, S, (({}, SCATTER if scatter else GATHER),), frames=(1,) if which == "r300" else (0, 1))


@pytest.mark.parametrize("which,S,scatter", C_LIMITS, ids=C_IDS)
def test_c_encode_at_the_limit(ctx, which, S, scatter):
    encode_case(ctx, which, S, (({}, STATIC if scatter else GATHER),), frames=(0,) if which == "r300" else (0, 1))


C_PKT = [("r300",) + p for p in zip(ar.edge_pair(ar.LIM_OFFSET, 300, 8), (True, False))] + \
        [("r64",) + p for p in zip(ar.edge_pair(ar.LIM_MUL24, 1, 8), (True, False))]


@pytest.mark.parametrize("which,S,fused", C_PKT, ids=[f"{w}-{S}-{'fused' if f else 'composed'}" for w, S, f in C_PKT])
def test_c_sender_at_the_limit(ctx, which, S, fused):
    """The packet-output encoder against n * (8 + S) < 2^32 and 8 + S < 2^24: the fused sender up to the limit, the composed path
    from it on, the same packets either way (F = 1: one frame is the whole range)."""
    c = cases.light_case(which)
    h, code = handle(ctx, which)
    n, k = code.n, code.k
    assert (n * (8 + S) < ar.LIM_OFFSET and 8 + S < ar.LIM_MUL24) == fused
    need((2 * n + k) * (8 + S) + GIB, f"sender ({n},{k}) F=1 S={S}")
    arn = Arena()
    src = tiled(arn, c["src"][:1], S)
    pk = poisoned(arn, (n, 8 + S))
    ctx.fec_encode_packets_device(h, src, 1, 250, out=pk)
    arn.check()
    info = ctx.fec_sender_info()
    print(f"[address-range] sender S={S}: {info} {apply_name(ctx)!r}")
    assert info["path"] == ("fused" if fused else "composed")
    if fused:
        assert apply_name(ctx).startswith(STATIC_PKT)
    bad = ar.lanes_mismatch(pk[:, 8:], dev(c["cw"][0]))
    assert bad is None, f"payload differs at (packet, tile, lane) {bad}"
    hdr = api.fec_packetize(np.zeros((1, n, 16), dtype=np.uint8), 1, 250)[:, :8]
    assert np.array_equal(pk[:, :8].cpu().numpy(), hdr), "headers"
    if fused:       # the composed path at the same size: same packets
        with knobs(ctx, {"ENC_PKT": "0"}):
            pk.fill_(POISON)
            ctx.fec_encode_packets_device(h, src, 1, 250, out=pk)
            arn.check()
            assert ctx.fec_sender_info()["path"] == "composed"
        assert ar.lanes_mismatch(pk[:, 8:], dev(c["cw"][0])) is None and np.array_equal(pk[:, :8].cpu().numpy(), hdr)


C_STRIDE_S = ar.last_below(ar.LIM_MUL24, 1, 8)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_c_flows_sender_stride_at_the_limit(ctx, fused):
    """The multi-flow sender against max_stride * (8 + S) < 2^32.  In round-robin order the stride is the number of flows, and a call
    holds stride * n packets, so the edge is in reach only with a tiny code and a long packet: a (3,1) code (two chained checks: a code with one check has no persistent encoder, so no fused sender), 8 + S just below 2^24,
    one frame per flow, 256 flows (fused: ldpc_scatter_static_flw_kernel) and 257 (composed).  Flow f sends frame f mod 2 of the
    small problem as block f mod 256."""
    S = C_STRIDE_S
    nflows = ar.stride_pair(S)[0 if fused else 1]
    c = cases.light_case("r3")
    h, code = handle(ctx, "r3")
    n, k, F = code.n, code.k, nflows
    assert (n, k) == (3, 1) and n * (8 + S) < ar.LIM_OFFSET and 8 + S < ar.LIM_MUL24
    assert (nflows * (8 + S) < ar.LIM_OFFSET) == fused
    need(F * (k * S + n * (8 + S)) + (1 << 29) + GIB, f"flows sender (3,1) S={S} flows={nflows}")
    arn = Arena()
    src = arn.new((F, k, S))
    small_src, small_cw = dev(c["src"]), dev(c["cw"])
    for r in range(2):
        part = src[r::2]
        ar.fill_lanes(part, small_src[r].unsqueeze(0).expand(part.shape[0], k, ar.P))
    pk = poisoned(arn, (F * n, 8 + S))
    blocks = np.arange(F) & 0xFF
    _, flow_of, _ = ctx.fec_encode_packets_flows_device(h, src, np.arange(F + 1), 1, blocks, api.TX_ROUND_ROBIN, out=pk)
    arn.check()
    info = ctx.fec_sender_flows_info()
    print(f"[address-range] flows sender stride={nflows}: {info} {apply_name(ctx)!r}")
    assert info["path"] == ("fused" if fused else "composed") and info["frames"] == F
    if fused:
        assert apply_name(ctx).startswith("ldpc_scatter_static_flw_kernel")
    # row j of flow f is packet j * nflows + f
    pkv = pk.view(n, F, 8 + S)
    for r in range(2):
        got = pkv[:, r::2, 8:]
        bad = ar.lanes_mismatch(got, small_cw[r].unsqueeze(1).expand(n, got.shape[1], ar.P))
        assert bad is None, f"payload of the flows {r}, {r + 2}, ...: (row, flow / 2, tile, lane) {bad}"
    hdr = np.array([[api.fec_header_pack(1, int(blocks[f]), j) for f in range(F)] for j in range(n)], dtype="<u8").view(np.uint8)
    assert np.array_equal(pkv[:, :, :8].cpu().numpy(), hdr.reshape(n, F, 8)), "headers"
    assert np.array_equal(flow_of.cpu().numpy(), np.tile(np.arange(F, dtype=np.int32), n)), "flow_of"
    assert ar.lanes_mismatch(src[0], small_src[0]) is None and ar.lanes_mismatch(src[F - 1], small_src[(F - 1) % 2]) is None


# ------------------------------------------------------------------------------------------------ D. Reed-Solomon (255,223)
D_S31 = ar.first_from(ar.LIM_SIGN, cases.RS_N)
D_FRAMES = ar.edge_pair(ar.LIM_RS_ROW)


def test_d_rs_encode_above_bit_31(ctx):
    """(rs_encode_kernel is the encoder's only kernel: there is no dispatch to observe.)"""
    c = cases.rs_case()
    n, k, S = cases.RS_N, cases.RS_K, D_S31
    assert n * S >= ar.LIM_SIGN
    need(2 * (n + k) * S + GIB, f"rs_encode B=2 S={S}")
    rs = ctx.rs_create(n, k)
    arn = Arena()
    src = tiled(arn, c["src"], S)
    cw = poisoned(arn, (2, n, S))
    assert ctx.rs_encode(rs, n, k, src, out=cw) is cw
    arn.check()
    bad = ar.lanes_mismatch(cw, dev(c["cw"]))
    assert bad is None, f"codeword differs at (block, row, tile, lane) {bad}"


@pytest.mark.parametrize("vw", [1, 2, 4])
def test_d_rs_decode_rows_above_bit_31(ctx, vw):
    """Gathered rows, the streaming kernel (S a multiple of 1024, so every RS_VW width is taken)."""
    c = cases.rs_case()
    n, k = cases.RS_N, cases.RS_K
    S = (ar.first_from(ar.LIM_SIGN, k) + 1023) // 1024 * 1024            # the rows of a block are [k][S]: k * S above 2^31
    assert k * S >= ar.LIM_SIGN and S % (256 * vw) == 0
    need(4 * k * S + GIB, f"rs_decode B=2 S={S} RS_VW={vw}")
    rs = ctx.rs_create(n, k)
    arn = Arena()
    val = tiled(arn, c["val"], S)
    idx = arn.new((2, 2 * k), src=c["idx"].view(np.uint8))
    msg = poisoned(arn, (2, k, S))
    with knobs(ctx, {"RS_VW": str(vw)} if vw != 1 else {}):
        ctx.rs_decode(rs, idx, val, out=msg)
        arn.check()
    name = ctx.rs_kernel_name()
    print(f"[address-range] rs_decode RS_VW={vw}: {name}")
    assert name == f"rs_decode_packets_kernel<{vw}, {2 if vw == 4 else 4}, false>", name       # the streaming kernel, this width
    assert ctx.rs_bad_blocks() == 0
    bad = ar.lanes_mismatch(msg, dev(c["msg"]))
    assert bad is None, f"message differs at (block, row, tile, lane) {bad}"


@pytest.mark.parametrize("S,streaming", list(zip(D_FRAMES, (True, False))), ids=[f"{D_FRAMES[0]}-streaming", f"{D_FRAMES[1]}-generic"])
def test_d_rs_decode_frames_at_the_limit(ctx, S, streaming):
    """Erased frames: block 0 misses r = 32 source symbols, block 1 is short.  Below 2^23 the streaming kernel's 24-bit row
    multiply holds; from 2^23 on the generic kernel runs."""
    assert (S < ar.LIM_RS_ROW) == streaming and S % 256 == 0
    c = cases.rs_case()
    n, k = cases.RS_N, cases.RS_K
    need(2 * (n + k) * S + 33 * S + GIB, f"rs_decode_frames B=2 S={S}")
    rs = ctx.rs_create(n, k)
    arn = Arena()
    sym, er = tiled(arn, c["fsym"], S), arn.new(c["fera"].shape, src=c["fera"])
    msg, recv, st = poisoned(arn, (2, k, S)), poisoned(arn, (2,), torch.int32), poisoned(arn, (2,), torch.int32)
    ctx.rs_decode_frames(rs, sym, er, out=(msg, recv, st))
    arn.check()
    name = ctx.rs_kernel_name()
    print(f"[address-range] rs_decode_frames S={S}: {name}")
    assert name == ("rs_decode_packets_kernel<1, 4, true>" if streaming else "rs_decode_kernel<true>"), name
    assert np.array_equal(recv.cpu().numpy(), c["received"]) and np.array_equal(st.cpu().numpy(), c["status"])
    bad = ar.lanes_mismatch(msg, dev(c["fmsg"]))
    assert bad is None, f"message differs at (block, row, tile, lane) {bad}"
    assert ar.lanes_mismatch(sym, dev(c["fsym"])) is None


# ------------------------------------------------------------------------------------------------ E. the batch axis
def frame_tiled(arn, small, F):
    return ar.fill_frames(arn.new((F,) + tuple(small.shape[1:])), dev(small))


def batch_words(got, want, F, tag):
    for name, a, b in zip(("sweeps", "residual", "status"), got, want):
        bad = ar.frames_mismatch(a, dev(b))
        assert bad is None, f"{tag}: {name} of frame {bad}"


def test_e_decode_s1_frames_beyond_2_32(ctx):
    c = cases.batch_case(1)
    h, code = handle(ctx, cases.B_CODE)
    n = code.n
    F = ar.frames_from(ar.LIM_OFFSET, n)
    need(3 * F * n + 16 * F + GIB, f"decode S=1 F={F}")
    arn = Arena()
    sym, er = frame_tiled(arn, c["sym"], F), frame_tiled(arn, c["era"], F)
    out, sw, res, st = poisoned(arn, (F, n)), *(poisoned(arn, (F,), torch.int32) for _ in range(3))
    ctx.decode(h, sym, er, out=out, sweeps=sw, residual=res, status=st)
    arn.check()
    names = ctx.profile_kernel_names()
    print("[address-range]", names)
    assert names["peel"].startswith("ldpc_peel") and names["apply"] == ""        # S = 1: the fused peel kernels, no packet kernel
    bad = ar.frames_mismatch(out, dev(c["want"][0]))
    assert bad is None, f"out of frame {bad}"
    batch_words((sw, res, st), c["want"][1:], F, "S=1")


def test_e_decode_1024_frames_beyond_2_32(ctx):
    S = 1024
    c = cases.batch_case(S)
    h, code = handle(ctx, cases.B_CODE)
    n = code.n
    F = ar.frames_from(ar.LIM_OFFSET, n * S)
    need(2 * F * n * S + 2 * GIB, f"decode S={S} F={F}")
    arn = Arena()
    sym, er = frame_tiled(arn, c["sym"], F), frame_tiled(arn, c["era"], F)
    out, sw, res, st = poisoned(arn, (F, n, S)), *(poisoned(arn, (F,), torch.int32) for _ in range(3))
    ctx.decode(h, sym, er, out=out, sweeps=sw, residual=res, status=st)
    arn.check()
    assert apply_name(ctx).startswith(SCATTER)
    bad = ar.frames_mismatch(out, dev(c["want"][0]))
    assert bad is None, f"out of frame {bad}"
    batch_words((sw, res, st), c["want"][1:], F, f"S={S}")
    ms = ctx.ml_stats()
    assert ms["residual_frames"] == int((ar.tile_frames(c["want"][3], F) != 0).sum())


def test_e_encode_and_packetize_1024_frames_beyond_2_32(ctx):
    """Encode, then the packetiser on its output: both arrays beyond 2^32 bytes."""
    S = 1024
    c = cases.batch_case(S)
    h, code = handle(ctx, cases.B_CODE)
    n, k = code.n, code.k
    F = ar.frames_from(ar.LIM_OFFSET, n * S)
    need(F * (k * S + n * S + n * (8 + S)) + GIB, f"encode + packetize S={S} F={F}")
    arn = Arena()
    src = frame_tiled(arn, c["src"], F)
    cw = poisoned(arn, (F, n, S))
    ctx.encode(h, src, out=cw)
    arn.check()
    assert apply_name(ctx).startswith(STATIC)
    bad = ar.frames_mismatch(cw, dev(c["cw"]))
    assert bad is None, f"codeword of frame {bad}"
    pk = poisoned(arn, (F * n, 8 + S))
    ctx.fec_packetize_device(cw, 1, 3, out=pk)
    arn.check()
    pkv = pk.view(F, n, 8 + S)
    bad = ar.frames_mismatch(pkv[:, :, 8:], dev(c["cw"]))
    assert bad is None, f"payload of frame {bad}"
    # headers: class 1, block (3 + f) mod 256, symbol j -- the host packetiser's words for 256 frames, tiled over the batch
    hdr = api.fec_packetize(np.zeros((256, n, 16), dtype=np.uint8), 1, 3)[:, :8].reshape(256, n, 8)
    bad = ar.frames_mismatch(pkv[:, :, :8], dev(hdr))
    assert bad is None, f"header of frame {bad}"


def test_e_receiver_packet_array_beyond_2_32(ctx):
    """The single-flow device receiver at one large S: decode_many over a packet array above 2^32 bytes (no loss, in order), the
    fused path -- the decoder fetches its rows from packets beyond 2^32."""
    which = "r300"
    c = cases.light_case(which)
    h, code = handle(ctx, which)
    n, k = code.n, code.k
    S = 1 << 20
    era, (_, w_sw, w_res, w_st) = c["era"][0], c["want"]
    assert w_st[0] in (0, 1) and np.array_equal(c["want"][0][0], c["cw"][0])     # frame 0's pattern is decodable
    kept = int((era == 0).sum())
    # the receiver keeps two blocks open: two blocks more than the array needs to have a CLOSED block start beyond 2^32 bytes
    B = ar.frames_from(ar.LIM_OFFSET, kept * (8 + S)) + 2
    need(B * (n + kept) * (8 + S) + (B + 2) * n * S + 2 * GIB, f"receiver ({n},{k}) S={S} blocks={B}")
    arn = Arena()
    # block b carries frame b mod 2 of the small problem's codewords (the oracle's), every block loses frame 0's erasure pattern
    small = dev(c["cw"])
    cwb = torch.empty((B, n, S), dtype=torch.uint8, device="cuda")
    for b in range(B):
        ar.fill_lanes(cwb[b], small[b % 2])
    full = ctx.fec_packetize_device(cwb, 1, 0)
    del cwb
    rows = dev(np.concatenate([b * n + np.nonzero(era == 0)[0] for b in range(B)]).astype(np.int64))
    pk = arn.new((B * kept, 8 + S))
    torch.index_select(full, 0, rows, out=pk)
    del full
    torch.cuda.empty_cache()
    out = poisoned(arn, (B, n, S))
    sw, res, st, rsrc = (poisoned(arn, (B,), torch.int32) for _ in range(4))
    eo = poisoned(arn, (B, n))
    rx = ctx.fec_rx_device(n, k, S)
    try:
        blocks, _, used = rx.decode_many(h, pk, B, out=(out, sw, res, st, eo, rsrc))
        nb = len(blocks)
        arn.check()
        info = ctx.fec_receiver_info()
        print("[address-range] receiver", info, apply_name(ctx), "blocks", blocks.tolist(), "used", used)
        assert info["path"] == "fused" and apply_name(ctx).startswith("ldpc_scatter_pktin_kernel")
        assert nb >= B - 2 and blocks.tolist() == list(range(nb)) and used == B * kept
        assert (nb - 1) * kept * (8 + S) >= ar.LIM_OFFSET                       # the last closed block starts beyond 2^32 bytes
        for name, a, w in (("sweeps", sw, w_sw), ("residual", res, w_res), ("status", st, w_st)):
            assert a[:nb].cpu().tolist() == [int(w[0])] * nb, name
        assert not bool(eo[:nb].any()) and not bool(rsrc[:nb].any())
        for b in range(nb):
            bad = ar.lanes_mismatch(out[b], small[b % 2])
            assert bad is None, f"block {b}: (row, tile, lane) {bad}"
        assert bool((out[nb:] == POISON).all()), "blocks that did not close were written"
    finally:
        rx.close()
