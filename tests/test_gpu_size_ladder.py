"""The size ladder (tools/size_ladder.py) through the C ABI with device pointers: registered codes that straddle the size switches of
the launch plans, every call either equal to the CPU oracle or refused cleanly.

One node per rung and symbol length (S = 1, 16, 256), smallest rung first.  A node encodes the batch and then, for every max_sweeps
the rung lists and ML on and off, runs decode, decode_frames (erased_out and residual_src) and the in-place decode.  Every input and
output lies between sentinel bands (Arena of tests/test_gpu_word_symbols.py) and every output is poisoned before every call.  The
erasure flags carry the values 1, 2, 0x80 and 0xFF; the expectation is made from the flags normalised to 0 / 1.

  rc == 0            out, sweeps, residual, status, erased_out and residual_src equal the oracle's on every frame (a status-3 frame
                     keeps its received symbols and holds the symbols the sweeps solved); encode equals OracleCode.encode
  rc == EUNSUP       every output byte and word is still the poison (in place: the frames are as they were), last_error names the
                     reason the host arithmetic gives (tools/size_ladder.host_plan), synchronize is OK and the same context then
                     decodes a small batch of built-in code 1 correctly
  any other rc       fails

A refusal is never accepted inside the envelope the project claims (n <= 8192, m <= 4096, row degree up to 16: decode at S = 1,
decode and encode on packets, ML on and off), and with do_ml = 0 never for a reason of the ML stage.  REFUSED is the refused share of
the ladder, 155 of 419 calls, every tuple written out: (rung, entry point, S, max_sweeps, do_ml, reason).  It was
recorded from a run on an MI355X and every entry agrees with host_plan; a change that refuses more (or less) has to change this list.

The last tests of the module look at what the nodes saw in last_plan() and profile_kernel_names(): every branch the ladder is built
to reach was reached ("Code sizes").  A node runs once per module, for whoever asks first: those tests run the nodes that
have not run yet, so they hold under -k and in any order.  Every packet encode is made twice, with the default schedule and with the
plain one (ENC_GROUP=0), which is the one that reads the encoder's compact lists."""
import itertools

import numpy as np
import pytest

import size_ladder_cases as cases
from ldpc_erasure_codes_amd import api, codes, synth
from size_ladder_cases import sl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_word_symbols import Arena  # noqa: E402

EUNSUP = -5
POISON = 0x5A
SIZES = (1, 16, 256)
ENTRIES = ("decode", "decode_frames", "inplace")
ML_CHECKS, ML_LDS, PEEL_LDS = "ML stage: more than 4096 checks", "ML stage: LDS need", "code too large for LDS"
GATHER_LDS, INPLACE_SCATTER = "gather kernel: LDS need", "in-place decode needs the scatter kernel"
E, D, F, I = "encode", "decode", "decode_frames", "inplace"   # noqa: E741
R0, R1, R2, R3 = "n8208_m4097_d8", "n11008_m5504_d16", "n16392_m8193_d8", "n49152_m4096_d8"
R4, R5, R6 = "n65534_m1024_d8", "n65534_m16384_d8", "n65534_m27307_d8"

# (rung, entry point, S, max_sweeps, do_ml, reason), every refused call written out; an encode has no max_sweeps or do_ml (0, 0)
REFUSED = sorted([
    # R0, m = 4097: the pivot key of the ML kernel has 12-bit row fields; everything with the ML stage off runs
    (R0, D, 1, 1, 1, ML_CHECKS), (R0, F, 1, 1, 1, ML_CHECKS), (R0, D, 1, 3, 1, ML_CHECKS), (R0, F, 1, 3, 1, ML_CHECKS),
    (R0, D, 1, 10, 1, ML_CHECKS), (R0, F, 1, 10, 1, ML_CHECKS), (R0, D, 16, 1, 1, ML_CHECKS), (R0, F, 16, 1, 1, ML_CHECKS),
    (R0, I, 16, 1, 1, ML_CHECKS), (R0, D, 16, 3, 1, ML_CHECKS), (R0, F, 16, 3, 1, ML_CHECKS), (R0, I, 16, 3, 1, ML_CHECKS),
    (R0, D, 16, 10, 1, ML_CHECKS), (R0, F, 16, 10, 1, ML_CHECKS), (R0, I, 16, 10, 1, ML_CHECKS), (R0, D, 256, 1, 1, ML_CHECKS),
    (R0, F, 256, 1, 1, ML_CHECKS), (R0, I, 256, 1, 1, ML_CHECKS), (R0, D, 256, 3, 1, ML_CHECKS), (R0, F, 256, 3, 1, ML_CHECKS),
    (R0, I, 256, 3, 1, ML_CHECKS), (R0, D, 256, 10, 1, ML_CHECKS), (R0, F, 256, 10, 1, ML_CHECKS), (R0, I, 256, 10, 1, ML_CHECKS),
    # R1, m = 5504, 16 entries per check: the ML stage again (its LDS plan fits with 32 bytes to spare); at max_sweeps = 10 the keys
    # of logM = 13 do not fit, and the serial kernel's packet plan (16 x 5504 x 2 bytes of tables) does not fit either
    (R1, D, 1, 3, 1, ML_CHECKS), (R1, F, 1, 3, 1, ML_CHECKS), (R1, D, 1, 10, 1, ML_CHECKS), (R1, F, 1, 10, 1, ML_CHECKS),
    (R1, D, 16, 3, 1, ML_CHECKS), (R1, F, 16, 3, 1, ML_CHECKS), (R1, I, 16, 3, 1, ML_CHECKS), (R1, D, 16, 10, 0, PEEL_LDS),
    (R1, F, 16, 10, 0, PEEL_LDS), (R1, I, 16, 10, 0, PEEL_LDS), (R1, D, 16, 10, 1, PEEL_LDS), (R1, F, 16, 10, 1, PEEL_LDS),
    (R1, I, 16, 10, 1, PEEL_LDS), (R1, D, 256, 3, 1, ML_CHECKS), (R1, F, 256, 3, 1, ML_CHECKS), (R1, I, 256, 3, 1, ML_CHECKS),
    (R1, D, 256, 10, 0, PEEL_LDS), (R1, F, 256, 10, 0, PEEL_LDS), (R1, I, 256, 10, 0, PEEL_LDS), (R1, D, 256, 10, 1, PEEL_LDS),
    (R1, F, 256, 10, 1, PEEL_LDS), (R1, I, 256, 10, 1, PEEL_LDS),
    # R2, m = 8193: no packet plan (8193 x 16 bytes of accumulators + tables > 160 KB) -- the gather kernel, never in place; keys fit
    # at max_sweeps = 1 only, behind that the serial kernel, whose packet plan does not fit
    (R2, D, 1, 1, 1, ML_LDS), (R2, F, 1, 1, 1, ML_LDS),
    (R2, D, 1, 3, 1, ML_LDS), (R2, F, 1, 3, 1, ML_LDS), (R2, D, 1, 10, 1, ML_LDS), (R2, F, 1, 10, 1, ML_LDS),
    (R2, I, 16, 1, 0, INPLACE_SCATTER), (R2, D, 16, 1, 1, ML_LDS), (R2, F, 16, 1, 1, ML_LDS), (R2, I, 16, 1, 1, INPLACE_SCATTER),
    (R2, D, 16, 3, 0, PEEL_LDS), (R2, F, 16, 3, 0, PEEL_LDS), (R2, I, 16, 3, 0, INPLACE_SCATTER), (R2, D, 16, 3, 1, PEEL_LDS),
    (R2, F, 16, 3, 1, PEEL_LDS), (R2, I, 16, 3, 1, INPLACE_SCATTER), (R2, D, 16, 10, 0, PEEL_LDS), (R2, F, 16, 10, 0, PEEL_LDS),
    (R2, I, 16, 10, 0, INPLACE_SCATTER), (R2, D, 16, 10, 1, PEEL_LDS), (R2, F, 16, 10, 1, PEEL_LDS),
    (R2, I, 16, 10, 1, INPLACE_SCATTER), (R2, I, 256, 1, 0, INPLACE_SCATTER), (R2, D, 256, 1, 1, ML_LDS),
    (R2, F, 256, 1, 1, ML_LDS), (R2, I, 256, 1, 1, INPLACE_SCATTER), (R2, D, 256, 3, 0, PEEL_LDS), (R2, F, 256, 3, 0, PEEL_LDS),
    (R2, I, 256, 3, 0, INPLACE_SCATTER), (R2, D, 256, 3, 1, PEEL_LDS), (R2, F, 256, 3, 1, PEEL_LDS),
    (R2, I, 256, 3, 1, INPLACE_SCATTER), (R2, D, 256, 10, 0, PEEL_LDS), (R2, F, 256, 10, 0, PEEL_LDS),
    (R2, I, 256, 10, 0, INPLACE_SCATTER), (R2, D, 256, 10, 1, PEEL_LDS), (R2, F, 256, 10, 1, PEEL_LDS),
    (R2, I, 256, 10, 1, INPLACE_SCATTER),
    # R3, n = 49152: past the relaxation; the serial kernel's packet plan needs 2 n bytes of state + 64 KB of tables.  S = 1 runs from
    # global tables with the ML stage off; the ML stage's plan (2 n bytes of column map) does not fit
    (R3, D, 1, 10, 1, ML_LDS), (R3, F, 1, 10, 1, ML_LDS), (R3, D, 16, 10, 0, PEEL_LDS),
    (R3, F, 16, 10, 0, PEEL_LDS), (R3, I, 16, 10, 0, INPLACE_SCATTER), (R3, D, 16, 10, 1, PEEL_LDS), (R3, F, 16, 10, 1, PEEL_LDS),
    (R3, I, 16, 10, 1, INPLACE_SCATTER), (R3, D, 256, 10, 0, PEEL_LDS), (R3, F, 256, 10, 0, PEEL_LDS),
    (R3, I, 256, 10, 0, INPLACE_SCATTER), (R3, D, 256, 10, 1, PEEL_LDS), (R3, F, 256, 10, 1, PEEL_LDS),
    (R3, I, 256, 10, 1, INPLACE_SCATTER),
    # R4, n = 65534, m = 1024: packets run (2 n of state + 16 KB of tables fit); S = 1 needs n more bytes for the codeword
    (R4, E, 1, 0, 0, PEEL_LDS), (R4, D, 1, 10, 0, PEEL_LDS), (R4, F, 1, 10, 0, PEEL_LDS),
    (R4, D, 1, 10, 1, PEEL_LDS), (R4, F, 1, 10, 1, PEEL_LDS),
    # R5, n = 65534, m = 16384: no decoder plan holds it; the packet encoder runs (gather kernel, 98 KB of LDS)
    (R5, E, 1, 0, 0, PEEL_LDS), (R5, D, 1, 1, 0, PEEL_LDS),
    (R5, F, 1, 1, 0, PEEL_LDS), (R5, D, 1, 1, 1, PEEL_LDS), (R5, F, 1, 1, 1, PEEL_LDS), (R5, D, 1, 10, 0, PEEL_LDS),
    (R5, F, 1, 10, 0, PEEL_LDS), (R5, D, 1, 10, 1, PEEL_LDS), (R5, F, 1, 10, 1, PEEL_LDS), (R5, D, 16, 1, 0, PEEL_LDS),
    (R5, F, 16, 1, 0, PEEL_LDS), (R5, I, 16, 1, 0, INPLACE_SCATTER), (R5, D, 16, 1, 1, PEEL_LDS), (R5, F, 16, 1, 1, PEEL_LDS),
    (R5, I, 16, 1, 1, INPLACE_SCATTER), (R5, D, 16, 10, 0, PEEL_LDS), (R5, F, 16, 10, 0, PEEL_LDS),
    (R5, I, 16, 10, 0, INPLACE_SCATTER), (R5, D, 16, 10, 1, PEEL_LDS), (R5, F, 16, 10, 1, PEEL_LDS),
    (R5, I, 16, 10, 1, INPLACE_SCATTER), (R5, D, 256, 1, 0, PEEL_LDS), (R5, F, 256, 1, 0, PEEL_LDS),
    (R5, I, 256, 1, 0, INPLACE_SCATTER), (R5, D, 256, 1, 1, PEEL_LDS), (R5, F, 256, 1, 1, PEEL_LDS),
    (R5, I, 256, 1, 1, INPLACE_SCATTER), (R5, D, 256, 10, 0, PEEL_LDS), (R5, F, 256, 10, 0, PEEL_LDS),
    (R5, I, 256, 10, 0, INPLACE_SCATTER), (R5, D, 256, 10, 1, PEEL_LDS), (R5, F, 256, 10, 1, PEEL_LDS),
    (R5, I, 256, 10, 1, INPLACE_SCATTER),
    # R6, n = 65534, m = 27307: the first m whose gather tables (6 m + 4 bytes) pass 160 KB -- nothing holds it
    (R6, E, 1, 0, 0, PEEL_LDS), (R6, D, 1, 10, 0, PEEL_LDS), (R6, F, 1, 10, 0, PEEL_LDS),
    (R6, D, 1, 10, 1, PEEL_LDS), (R6, F, 1, 10, 1, PEEL_LDS), (R6, E, 16, 0, 0, GATHER_LDS), (R6, D, 16, 10, 0, PEEL_LDS),
    (R6, F, 16, 10, 0, PEEL_LDS), (R6, I, 16, 10, 0, INPLACE_SCATTER), (R6, D, 16, 10, 1, PEEL_LDS), (R6, F, 16, 10, 1, PEEL_LDS),
    (R6, I, 16, 10, 1, INPLACE_SCATTER), (R6, E, 256, 0, 0, GATHER_LDS), (R6, D, 256, 10, 0, PEEL_LDS),
    (R6, F, 256, 10, 0, PEEL_LDS), (R6, I, 256, 10, 0, INPLACE_SCATTER), (R6, D, 256, 10, 1, PEEL_LDS),
    (R6, F, 256, 10, 1, PEEL_LDS), (R6, I, 256, 10, 1, INPLACE_SCATTER),
])
REFUSED_KEYS = {t[:5]: t[5] for t in REFUSED}
_NODES = {}        # (rung, S) -> one dict per call of that node (run_rung)
_KNOBS = {}        # rung -> (S, knob) of the knob cross-checks that ran both variants (run_knobs)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


_HANDLES = {}


def handle(ctx, name):
    if (id(ctx), name) not in _HANDLES:
        _HANDLES[(id(ctx), name)] = ctx.register_code(cases.rung_case(name)["code"])
    return _HANDLES[(id(ctx), name)]


def small_builtin_batch(ctx, oracle):
    """built-in code 1, four frames at S = 1 through the host-pointer path, against the oracle"""
    if "small" not in _HANDLES:
        code = codes.load_builtin(1)
        era = synth.erasures_uniform(11, 0, 4, code.n, 0.12)
        sym = synth.source(12, 0, 4, code.n, 1)[:, :, 0].copy()
        _HANDLES["small"] = (ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1]), sym, era,
                             oracle.OracleCode(code).decode_batch_s1(sym, era))
    h, sym, era, want = _HANDLES["small"]
    for a, b in zip(ctx.decode(h, sym, era), want):
        assert np.array_equal(a, b), "the context does not decode correctly after a refusal"


def poisoned(ar, shape, dtype=torch.uint8):
    t = ar.new(shape, dtype)
    t.view(torch.uint8).fill_(POISON)
    return t


def is_poison(t):
    return bool((t.contiguous().view(torch.uint8) == POISON).all())


def frame_shape(F, rows, S):
    return (F, rows) if S == 1 else (F, rows, S)


def run_decode(ctx, h, entry, S, sym_host, dera, max_sweeps, do_ml, ar, dsym=None):
    """One call.  Returns (rc, dict of device outputs, the input tensor).  in place: a fresh copy of the frames is input and output."""
    F, n = sym_host.shape[0], sym_host.shape[1]
    inplace = entry == "inplace"
    if inplace or dsym is None:
        dsym = ar.new(sym_host.shape, src=sym_host)
    o = {"out": dsym if inplace else poisoned(ar, sym_host.shape)}
    for name in ("sweeps", "residual", "status"):
        o[name] = poisoned(ar, (F,), torch.int32)
    L = ctx._L
    if entry == "decode":
        rc = L.ldpc_amd_decode_batch(ctx._h, h, S, F, dsym.data_ptr(), dera.data_ptr(), max_sweeps, do_ml, o["out"].data_ptr(),
                                     o["sweeps"].data_ptr(), o["residual"].data_ptr(), o["status"].data_ptr(), api.DEVICE_PTRS)
    else:
        o["erased_out"] = poisoned(ar, (F, n))
        o["residual_src"] = poisoned(ar, (F,), torch.int32)
        rc = L.ldpc_amd_decode_frames(ctx._h, h, S, F, dsym.data_ptr(), dera.data_ptr(), max_sweeps, do_ml, o["out"].data_ptr(),
                                      o["sweeps"].data_ptr(), o["residual"].data_ptr(), o["status"].data_ptr(), o["erased_out"].data_ptr(),
                                      o["residual_src"].data_ptr(), api.DEVICE_PTRS | (api.INPLACE if inplace else 0))
    return rc, o, dsym


def check_refusal(ctx, oracle, rc, outs, tag, reason, unchanged=None):
    """the refusal is clean: nothing was written, the reason is named, the context works on"""
    assert rc == EUNSUP, (tag, rc, ctx._L.ldpc_amd_last_error(ctx._h))
    text = ctx._L.ldpc_amd_last_error(ctx._h).decode()
    torch.cuda.synchronize()
    for name, t in outs.items():
        if unchanged is not None and name == "out":
            assert np.array_equal(t.cpu().numpy(), unchanged), f"{tag}: a refused in-place call changed the frames ({text})"
        else:
            assert is_poison(t), f"{tag}: a refused call wrote to {name} ({text})"
    assert reason is not None and text.startswith(reason), f"{tag}: refused with '{text}', the host arithmetic says '{reason}'"
    ctx.synchronize()
    small_builtin_batch(ctx, oracle)


def check_equal(outs, w, S, tag):
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    F, n = w.out.shape[0], w.out.shape[1]
    for name in ("sweeps", "residual", "status") + (("erased_out", "residual_src") if "erased_out" in host else ()):
        bad = np.flatnonzero((host[name] != getattr(w, name)).reshape(F, -1).any(1))
        assert bad.size == 0, f"{tag}: {name} differs in frames {bad.tolist()}: {host[name][bad].tolist()[:4]} != {getattr(w, name)[bad].tolist()[:4]}"
    # a status-3 frame: what was received or solved by the sweeps; every other frame: every byte
    open_ = (w.status == 3)[:, None] & (w.erased_out != 0)
    diff = (host["out"].reshape(F, n, S) != w.out).any(2) & ~open_
    bad = np.flatnonzero(diff.any(1))
    assert bad.size == 0, f"{tag}: out differs in frames {bad.tolist()} (status {w.status[bad].tolist()}), first symbols {np.flatnonzero(diff[bad[0]])[:8].tolist()}"


def host_plan(c, entry, S, ms, ml):
    f = c["facts"]
    return sl.host_plan(c["rung"].n, c["rung"].m, f["maxdeg"], f["maxcoldeg"], entry, S, ms, ml)


def in_envelope(rung):
    return rung.n <= 8192 and rung.m <= 4096 and rung.deg <= 16


# ------------------------------------------------------------------------------------------------ the rungs
def run_rung(ctx, oracle, name, S):
    """One node: every call of the rung at this S.  Returns its records (one dict per call); a node runs once per module, whoever
    asks first -- its own test or the tests of the whole ladder below, which therefore do not depend on what ran before them."""
    if (name, S) in _NODES:
        return _NODES[(name, S)]
    OBSERVED = []
    c, s = cases.rung_case(name), cases.symbols(name, S)
    rung, code, b, F = c["rung"], c["code"], c["batch"], s["F"]
    n, k = code.n, code.k
    h = handle(ctx, name)
    squeeze = (lambda a: np.ascontiguousarray(a[:, :, 0])) if S == 1 else (lambda a: a)
    ar = Arena()

    # ---- encode
    tag = f"{name} encode S={S}"
    dsrc = ar.new(frame_shape(F, k, S), src=squeeze(s["src"]))
    dcw = poisoned(ar, frame_shape(F, n, S))
    rc = ctx._L.ldpc_amd_encode_batch(ctx._h, h, S, F, dsrc.data_ptr(), dcw.data_ptr(), api.DEVICE_PTRS)
    hp = host_plan(c, "encode", S, 0, 0)
    rec = dict(rung=name, entry="encode", S=S, max_sweeps=0, do_ml=0, rc=rc, host=hp)
    if rc == 0:
        ctx.synchronize()
        got = dcw.cpu().numpy().reshape(F, n, S)
        bad = np.flatnonzero((got != s["cw"]).reshape(F, -1).any(1))
        assert bad.size == 0, f"{tag}: frames {bad.tolist()} differ from OracleCode.encode"
        rec["kernel"] = ctx.encode_kernel_name() if S > 1 else ctx.profile_kernel_names()["peel"]
        scatter = S > 1 and rec["kernel"].startswith("ldpc_scatter")       # (the gather kernel has one schedule and leaves the word alone)
        rec["grouped"] = ctx.encode_info(h)["last_encode_grouped"] if scatter else 0
        if S > 1:   # ... and with the plain schedule (ENC_GROUP=0), the one that reads the compact lists where the code kept them
            ctx.configure("LDPC_AMD_ENC_GROUP", "0")
            try:
                dcw2 = poisoned(ar, frame_shape(F, n, S))
                rc2 = ctx._L.ldpc_amd_encode_batch(ctx._h, h, S, F, dsrc.data_ptr(), dcw2.data_ptr(), api.DEVICE_PTRS)
                assert rc2 == 0, (tag, "ENC_GROUP=0", ctx._L.ldpc_amd_last_error(ctx._h))
                ctx.synchronize()
                bad = np.flatnonzero((dcw2.cpu().numpy().reshape(F, n, S) != s["cw"]).reshape(F, -1).any(1))
                assert bad.size == 0, f"{tag} ENC_GROUP=0: frames {bad.tolist()} differ from OracleCode.encode"
                rec["plain_kernel"] = ctx.encode_kernel_name()
                assert not scatter or ctx.encode_info(h)["last_encode_grouped"] == 0
            finally:
                ctx.configure("LDPC_AMD_ENC_GROUP", None)
    else:
        assert not in_envelope(rung), f"{tag}: refused inside the claimed envelope: {ctx._L.ldpc_amd_last_error(ctx._h)}"
        check_refusal(ctx, oracle, rc, {"codeword": dcw}, tag, hp["refused"])
    ar.check()
    assert np.array_equal(dsrc.cpu().numpy(), squeeze(s["src"])), f"{tag}: the source was written"
    OBSERVED.append(rec)
    assert (rc != 0) == ((name, "encode", S, 0, 0) in REFUSED_KEYS), f"{tag}: rc {rc} against the recorded refused list"

    # ---- decode, decode_frames, in place
    sym = squeeze(s["sym"])
    dera = ar.new(b.flags.shape, src=b.flags)             # flags 1, 2, 0x80, 0xFF
    dsym = ar.new(sym.shape, src=sym)
    for ms, ml, entry in itertools.product(rung.sweeps, (0, 1), ENTRIES):
        if entry == "inplace" and S == 1:
            continue
        tag = f"{name} {entry} S={S} max_sweeps={ms} do_ml={ml}"
        rc, outs, din = run_decode(ctx, h, entry, S, sym, dera, ms, ml, ar, dsym)
        hp = host_plan(c, entry, S, ms, ml)
        rec = dict(rung=name, entry=entry, S=S, max_sweeps=ms, do_ml=ml, rc=rc, host=hp)
        if rc == 0:
            ctx.synchronize()
            check_equal(outs, cases.want(name, S, ms, ml), S, tag)
            rec["plan"] = ctx.last_plan()
            names = ctx.profile_kernel_names()
            rec["peel"], rec["apply"] = names["peel"], (names["apply"] if S > 1 else "")
        else:
            text = ctx._L.ldpc_amd_last_error(ctx._h).decode()
            assert not in_envelope(rung), f"{tag}: refused inside the claimed envelope: {text}"
            assert ml or not text.startswith("ML stage"), f"{tag}: refused for the ML stage with the ML stage off: {text}"
            check_refusal(ctx, oracle, rc, outs, tag, hp["refused"], unchanged=sym if entry == "inplace" else None)
        ar.check()
        if entry != "inplace":
            assert np.array_equal(din.cpu().numpy(), sym), f"{tag}: an out-of-place decode wrote to its input"
        OBSERVED.append(rec)
        assert (rc != 0) == ((name, entry, S, ms, ml) in REFUSED_KEYS), f"{tag}: rc {rc} against the recorded refused list"
    assert np.array_equal(dera.cpu().numpy(), b.flags), f"{name} S={S}: the flags were written"
    assert ctx.knobs() == ""
    _NODES[(name, S)] = OBSERVED
    return OBSERVED


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("name", [r.name for r in sl.RUNGS])
def test_rung(ctx, oracle, name, S):
    run_rung(ctx, oracle, name, S)


# ------------------------------------------------------------------------------------------------ both variants of a kernel choice
KNOB_RUNGS = ("n4104_m1026", "n8192_m4096_d8", "n8192_m4096_d14", "n8208_m4097_d8", "n32767_m2047_d8", "n65534_m1024_d8")


def run_knobs(ctx, oracle, name):
    """PEEL_RELAX=0 (the serial kernel where the relaxation runs) and APPLY=gather (the gather kernel where the packet kernel runs)
    against the default, decode_frames: every byte and word equal -- the open symbols of a status-3 frame included, which the
    oracle does not pin.  Where a variant has no plan of its own for the rung it must refuse cleanly."""
    if name in _KNOBS:
        return _KNOBS[name]
    COMPARED = []
    c = cases.rung_case(name)
    rung, b = c["rung"], c["batch"]
    h = handle(ctx, name)
    for S in SIZES:
        s = cases.symbols(name, S)
        sym = np.ascontiguousarray(s["sym"][:, :, 0]) if S == 1 else s["sym"]
        ar = Arena()
        dera, dsym = ar.new(b.flags.shape, src=b.flags), ar.new(sym.shape, src=sym)
        served = [(ms, ml) for ml in (1, 0) for ms in rung.sweeps[::-1] if (name, "decode_frames", S, ms, ml) not in REFUSED_KEYS]
        if not served:      # (n = 65534 at S = 1: no variant runs)
            continue
        ms, ml = served[0]
        rc, ref, _ = run_decode(ctx, h, "decode_frames", S, sym, dera, ms, ml, ar, dsym)
        assert rc == 0
        ctx.synchronize()
        ref = {k_: v.cpu().numpy() for k_, v in ref.items()}
        for knob, value in (("LDPC_AMD_PEEL_RELAX", "0"),) + ((("LDPC_AMD_APPLY", "gather"),) if S > 1 else ()):
            tag = f"{name} S={S} max_sweeps={ms} do_ml={ml} {knob}={value}"
            ctx.configure(knob, value)
            try:
                rc, outs, _ = run_decode(ctx, h, "decode_frames", S, sym, dera, ms, ml, ar, dsym)
                if rc == 0:
                    ctx.synchronize()
                    check_equal(outs, cases.want(name, S, ms, ml), S, tag)
                    for k_, v in outs.items():
                        assert np.array_equal(v.cpu().numpy(), ref[k_]), f"{tag}: {k_} differs from the default"
                    COMPARED.append((S, knob))
                else:
                    text = ctx._L.ldpc_amd_last_error(ctx._h).decode()
                    check_refusal(ctx, oracle, rc, outs, tag, text.split(" (")[0])
                    assert text.startswith(PEEL_LDS), tag    # (the serial kernel is the one that would run: its plan counts)
            finally:
                ctx.configure(knob, None)
            ar.check()
    assert ctx.knobs() == ""
    _KNOBS[name] = COMPARED
    return COMPARED


@pytest.mark.parametrize("name", KNOB_RUNGS)
def test_knob_variants_equal_the_default(ctx, oracle, name):
    run_knobs(ctx, oracle, name)


# ------------------------------------------------------------------------------------------------ what the ladder saw
@pytest.fixture(scope="module")
def observed(ctx, oracle):
    """every call of the ladder, rung by rung (nodes that have run already are not run again)"""
    return [o for r in sl.RUNGS for S in SIZES for o in run_rung(ctx, oracle, r.name, S)]


def _where(observed, pred):
    return [(o["rung"], o["entry"], o["S"], o["max_sweeps"], o["do_ml"]) for o in observed if o["rc"] == 0 and pred(o)]


def test_refused_share_is_the_recorded_list(observed):
    OBSERVED = observed
    ncalls = sum(3 + len(r.sweeps) * 2 * (2 + 3 + 3) for r in sl.RUNGS)
    assert len(OBSERVED) == ncalls == 419
    assert all(o["rc"] in (0, EUNSUP) for o in OBSERVED)
    got = sorted((o["rung"], o["entry"], o["S"], o["max_sweeps"], o["do_ml"], o["host"]["refused"]) for o in OBSERVED if o["rc"] != 0)
    assert got == REFUSED
    assert len(REFUSED) == 155
    assert not [t for t in REFUSED if in_envelope(sl.BY_NAME[t[0]])]
    assert not [t for t in REFUSED if t[1] != "encode" and t[4] == 0 and t[5].startswith("ML stage")]


def test_every_branch_of_the_plans_was_reached(ctx, oracle, observed):
    OBSERVED = observed
    _seen = lambda pred: _where(observed, pred)                                       # noqa: E731
    dec = lambda o: o["entry"] != "encode"                                            # noqa: E731
    relax = lambda o: dec(o) and o["peel"].startswith("ldpc_peel_relax_kernel<")      # noqa: E731
    serial = lambda o: dec(o) and o["peel"].startswith("ldpc_peel_kernel<")           # noqa: E731
    packet = lambda o: dec(o) and o["S"] > 1 and o["apply"].startswith("ldpc_scatter_kernel<")   # noqa: E731
    seen = {
        "relaxation, tables in LDS": _seen(lambda o: relax(o) and not o["plan"]["tables_in_global"]),
        "relaxation, global tables forced by size": _seen(lambda o: relax(o) and o["plan"]["tables_in_global"] and o["host"]["tables_in_global"]),
        "fused serial kernel with global tables": _seen(lambda o: dec(o) and o["S"] == 1 and o["peel"] in ("ldpc_peel_kernel<8, true, true>", "ldpc_peel_kernel<16, true, true>")),
        "serial kernel because the keys do not fit": _seen(lambda o: serial(o) and o["host"]["why_serial"] == "keys"),
        "serial kernel because n > 32767": _seen(lambda o: serial(o) and o["host"]["why_serial"] == "n"),
        "two tiers on": _seen(lambda o: packet(o) and o["plan"]["two_tiers"] == 1),
        "two tiers off because of size": _seen(lambda o: packet(o) and o["plan"]["two_tiers"] == 0 and o["plan"]["packet_bytes_per_workgroup"] < 128),
        "gather kernel for want of a packet plan, light columns": _seen(lambda o: dec(o) and o["S"] > 1 and o["apply"] == "ldpc_apply_kernel" and
                                                                          cases.rung_case(o["rung"])["facts"]["maxcoldeg"] <= 16),
    }
    for B in (16, 32, 64, 128, 256):
        seen["packet kernel, %d bytes per workgroup" % B] = _seen(lambda o: packet(o) and o["plan"]["packet_bytes_per_workgroup"] == B)
    # The encoder's compact lists (api.cpp: enc_lst, the lists of the parity symbols without each one's own check): 16-bit offsets,
    # so a code with 65535 entries or more drops them at registration.  The plain schedule (ENC_GROUP=0) is the one that reads them.
    # KEPT is seen: the persistent encoder runs the plain schedule only with them (launch_scatter_lpr: enc_group || enc_clist).
    # DROPPED has no outlet of its own in the ABI: the count below is registration's rule applied to the rung's code, and what is
    # observed is that the scatter encoder -- never the persistent one -- runs the plain schedule on that code and equals the oracle.
    lst = lambda o: cases.rung_case(o["rung"])["facts"]["enc_lst"]                                                                     # noqa: E731
    plain = lambda o: o["entry"] == "encode" and o["S"] > 1 and o.get("plain_kernel", "").startswith("ldpc_scatter")                     # noqa: E731
    seen["scatter encoder, plain schedule, compact lists dropped"] = _seen(lambda o: plain(o) and lst(o) >= 65535 and
                                                                           o["plain_kernel"].startswith("ldpc_scatter_kernel<"))
    seen["scatter encoder, plain schedule, compact lists kept"] = _seen(lambda o: plain(o) and 0 < lst(o) < 65535 and
                                                                        o["plain_kernel"].startswith("ldpc_scatter_static_kernel<"))
    assert max(lst(o) for o in OBSERVED) >= 65535 > sorted({lst(o) for o in OBSERVED})[-2], "one rung past the 16-bit offsets, the others well below"
    for o in OBSERVED:      # the table of DESIGN.md section 4.7 (pytest -s)
        if o["entry"] in ("encode", "decode"):
            what = "refused: " + str(o["host"]["refused"]) if o["rc"] else ("%s grouped %d | plain: %s" % (o["kernel"], o["grouped"], o.get("plain_kernel", "-")) if o["entry"] == "encode" else "%s %s %s" % (
                o["peel"], o["apply"], {k_: o["plan"][k_] for k_ in ("tables_in_global", "packet_bytes_per_workgroup", "two_tiers")}))
            print("%-18s %-6s S %3d sweeps %2d ml %d  %s" % (o["rung"], o["entry"], o["S"], o["max_sweeps"], o["do_ml"], what))
    for what, where in seen.items():
        print("%-56s %3d calls, first %s" % (what, len(where), where[:1]))
    missing = [what for what, where in seen.items() if not where]
    assert not missing, missing
    # the host arithmetic the refused list was checked against is the library's: same peel kernel, same packet plan on every call that ran
    for o in OBSERVED:
        if o["rc"] == 0 and dec(o):
            hp, tag = o["host"], (o["rung"], o["entry"], o["S"], o["max_sweeps"], o["do_ml"])
            assert (hp["peel"] == "relax") == o["peel"].startswith("ldpc_peel_relax_kernel<"), tag
            if o["S"] > 1:
                assert hp["packet_bytes"] == o["plan"]["packet_bytes_per_workgroup"] and hp["two_tiers"] == bool(o["plan"]["two_tiers"]), tag
    COMPARED = [t for name in KNOB_RUNGS for t in run_knobs(ctx, oracle, name)]
    assert {k_ for _, k_ in COMPARED} == {"LDPC_AMD_PEEL_RELAX", "LDPC_AMD_APPLY"}, COMPARED
    assert any(S == 1 for S, k_ in COMPARED if k_ == "LDPC_AMD_PEEL_RELAX") and any(S > 1 for S, k_ in COMPARED if k_ == "LDPC_AMD_PEEL_RELAX")


# ------------------------------------------------------------------------------------------------ erasure flags: non-zero = erased
def test_erasure_flags_any_nonzero_value(ctx):
    """include/ldpc_erasure_amd.h: "non-zero = erased".  The same call with flags drawn from {1, 2, 0x80, 0xFF} and with those
    flags normalised to 0 / 1: all outputs identical, and erased_out holds 0 and 1 only.  decode at S = 1 with the flag array 8-byte
    aligned (64-bit flag loads) and at an odd byte offset (byte path), decode at S = 16 and 256, decode_frames, in place,
    rs_decode_frames; host and device pointers."""
    code = codes.load_builtin(1)
    n, k = code.n, code.k
    h = ctx.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
    era01 = np.concatenate([synth.erasures_uniform(21, 0, 2, n, p) for p in (0.10, 0.22, 0.26)])     # sweeps alone, ML stage, ML stage
    F = era01.shape[0]
    vals = np.array(sl.FLAG_VALUES, dtype=np.uint8)[(np.arange(n)[None, :] * 3 + np.arange(F)[:, None]) % 4]
    era = np.where(era01 != 0, vals, 0).astype(np.uint8)
    assert set(np.unique(era).tolist()) == {0, 1, 2, 0x80, 0xFF}

    def same(a, b, tag):
        for i, (x, y) in enumerate(zip(a, b)):
            x, y = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (x, y))
            assert np.array_equal(x, y), f"{tag}: output {i} depends on the value of a non-zero flag"

    def offset_copy(a, off):
        """device copy of `a` whose first byte lies `off` bytes behind an 8-byte aligned address"""
        big = torch.empty(a.size + 16, dtype=torch.uint8, device="cuda")
        assert big.data_ptr() % 8 == 0
        t = big[off:off + a.size].view(a.shape)
        t.copy_(torch.from_numpy(np.array(a)))
        assert t.data_ptr() % 8 == off
        return t

    for S in (1, 16, 256):
        src = synth.source(30 + S, 0, F, k, S)
        cw = ctx.encode(h, src[:, :, 0] if S == 1 else src)
        sym = cw.copy()
        sym[era01.astype(bool)] = 0x77
        for do_ml in (1, 0):
            tag = f"S={S} do_ml={do_ml}"
            ref = ctx.decode_frames(h, sym, era01, do_ml=do_ml)
            assert set(np.unique(ref.erased_out).tolist()) <= {0, 1} and set(ref.status.tolist()) >= ({0, 1} if do_ml else {0, 3})
            same(ctx.decode(h, sym, era, do_ml=do_ml), ref[:4], tag + " decode host")
            same(ctx.decode_frames(h, sym, era, do_ml=do_ml), ref, tag + " decode_frames host")
            dsym = torch.from_numpy(sym).cuda()
            for off in (0, 1, 5) if S == 1 else (0, 3):
                for flags in (era, era01):
                    d = offset_copy(flags, off)
                    same(ctx.decode(h, dsym, d, do_ml=do_ml), ref[:4], tag + f" decode device, flags at +{off}")
                    r = ctx.decode_frames(h, dsym, d, do_ml=do_ml)
                    ctx.synchronize()
                    same(r, ref, tag + f" decode_frames device, flags at +{off}")
                    assert set(np.unique(r.erased_out.cpu().numpy()).tolist()) <= {0, 1}
                    if S > 1:
                        r = ctx.decode_frames(h, dsym.clone(), d, do_ml=do_ml, inplace=True)
                        ctx.synchronize()
                        same(r[1:], ref[1:], tag + f" in place, flags at +{off}")
                        open_ = (ref.status == 3)[:, None] & (ref.erased_out != 0)       # (in place an open symbol keeps what the caller left there)
                        assert not ((r.out.cpu().numpy() != ref.out).any(2) & ~open_).any(), tag + " in place: out"

    # Reed-Solomon decode from erased frames
    rn, rk = code.rs_n, code.rs_k
    rs = ctx.rs_create(rn, rk)
    rng = np.random.default_rng(5)
    B = 6
    rera01 = (rng.random((B, rn)) < 0.15).astype(np.uint8)
    rera01[B - 1, :rn - rk + 3] = 1                                                    # one block short of k symbols
    rvals = np.array(sl.FLAG_VALUES, dtype=np.uint8)[(np.arange(rn)[None, :] + np.arange(B)[:, None]) % 4]
    rera = np.where(rera01 != 0, rvals, 0).astype(np.uint8)
    for S in (1, 16):
        msg = rng.integers(0, 256, size=(B, rk, S), dtype=np.uint8)
        rcw = ctx.rs_encode(rs, rn, rk, msg[:, :, 0].copy() if S == 1 else msg)
        rsym = rcw.copy()
        rsym[rera01.astype(bool)] = 0x77
        ref = ctx.rs_decode_frames(rs, rsym, rera01)
        assert np.array_equal(ref.msg[:B - 1].reshape(B - 1, rk, S), msg[:B - 1]) and len(set(ref.status.tolist())) == 2
        same(ctx.rs_decode_frames(rs, rsym, rera), ref, f"rs_decode_frames host S={S}")
        for off in (0, 1):
            r = ctx.rs_decode_frames(rs, torch.from_numpy(rsym).cuda(), offset_copy(rera, off))
            ctx.synchronize()
            same(r, ref, f"rs_decode_frames device S={S}, flags at +{off}")
    assert ctx.knobs() == ""
