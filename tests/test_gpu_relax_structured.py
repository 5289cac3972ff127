"""The time-stamp relaxation (csrc/peel_relax.inc) on chain-structured codes, GPU, through the C-ABI.

The other suites reach the relaxation with the built-in codes and random codes under uniform erasures, where it settles in a
few dozen rounds.  Here: the families of tools/relax_model.py -- staircase (dual-diagonal) parity parts up to m = 4096, sizes
that are no multiple of 64 or of 8, fewer checks than a wavefront, chains that restart inside a chunk of 64 checks, chains
against the sweep order, the chained random triangle code -- and the built-in codes, under the structured erasure patterns of
relax_model.structured_erasures (all parity, a run across a chunk border, every second parity symbol, residuals of full and of
deficient rank, all clear, all erased), a third of the frames not codewords.  tests/test_relax_model_cpu.py replays the
kernel's loop on the same inputs and shows what they cost: about m rounds, beyond the safety cap the loop had in round 4.

Every combination of sweep cap (1, 3, 10, the largest whose keys fit 16 bits, one above it: the fall-back), ML stage on / off,
S = 1 / 64 / 1024, code tables in LDS / global memory (PEEL_GT), plain / paired levels (SCATTER_PAIRS) and forced tier-2 pieces
(SCATTER_T2P_FORCE) is decoded with PEEL_RELAX = 1 and 0.  The two must agree on every byte and status word, and both must
equal the oracle (Matlab/My_LDPC_HybridML_NonBinary_Erasure_Decoder.m:13-129) on EVERY frame.  A PEEL_RELAX = 1 decode must have
run a relaxation kernel exactly when the keys fit: a silent fall-back to the serial kernel does not pass."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import relax_model as rm  # noqa: E402

from ldpc_erasure_codes_amd import api, codes, synth  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(rm.FAMILIES) + ["builtin_%d" % i for i in rm.BUILTIN]
WHAT = ("out", "sweeps", "residual", "status")


def _oracle_frames(oc, sym, era, S, sweeps, do_ml):
    """Per frame: (bytes [n, S], symbols still unknown [n], iterations, residual count, status word)."""
    exp = []
    for f in range(sym.shape[0]):
        o_out, o_unk, o_it, info, rc = oc.decode_packets(sym[f].reshape(oc.n, S), era[f], itenum=sweeps, do_ml=do_ml)
        want = 0 if info[0] == 0 else (3 if (rc == -2 or not info[1]) else (2 if info[2] else 1))
        exp.append((o_out, o_unk.astype(bool), o_it, int(info[0]), want))
    return exp


def _equals_the_oracle(got, exp, sym, era, S, what):
    out, sw, res, st = got
    n = sym.shape[1]
    for f, (o_out, o_unk, o_it, o_res, want) in enumerate(exp):
        ctxt = what + (f, rm.PATTERNS[f % len(rm.PATTERNS)])
        assert (int(sw[f]), int(res[f]), int(st[f])) == (o_it, o_res, want), (ctxt, sw[f], o_it, res[f], o_res, st[f], want)
        g = out[f].reshape(n, S)
        if want != 3:
            assert np.array_equal(g, o_out), ctxt
        else:   # ML not run: what was received stays as it is, what the sweeps solved is the oracle's
            known = era[f] == 0
            solved = ~known & ~o_unk
            assert np.array_equal(g[known], sym[f].reshape(n, S)[known]), ctxt
            assert np.array_equal(g[solved], o_out[solved]), ctxt


def _knob_sets(S):
    if S == 1:
        return [{"PEEL_GT": gt} for gt in ("0", "1")]
    return [{"PEEL_GT": gt, "SCATTER_PAIRS": pairs, "SCATTER_T2P_FORCE": force}
            for gt in ("0", "1") for pairs in ("0", "1") for force in ("0", "1")]


@pytest.mark.parametrize("name", CASES)
def test_structured_codes_relaxation_serial_loop_and_oracle_agree(oracle, name):
    if name.startswith("builtin_"):
        ind = int(name[len("builtin_"):])
        if not codes.have_builtin(ind):
            pytest.skip("fixture of this code not present")
        code = codes.load_builtin(ind, codes.DEFAULT_COEF_SEED[ind])
    else:
        ind, code = None, rm.family_code(name)
    oc = oracle.OracleCode(code)
    n, k, m = code.n, code.k, code.m
    triangle = rm.is_triangle(code)
    seed = 300 + CASES.index(name)
    rng = np.random.default_rng(seed)
    # every pattern once at m = 4096 (8 frames), three times with other runs and source symbols elsewhere (24 frames)
    era = np.concatenate([rm.structured_erasures(rng, code) for _ in range(1 if m >= 4096 else 3)])
    F = era.shape[0]
    assert F <= (8 if m >= 4096 else 24)
    top = rm.largest_fitting_sweeps(m)
    caps = rm.sweep_caps(m) + [top + 1]
    assert all(rm.fits(m, s) for s in caps[:-1]) and not rm.fits(m, top + 1)
    seen = set()
    with api.Context(0) as ctx:
        h = ctx.register_code(code) if ind is None else ctx.load_builtin_code(ind, codes.DEFAULT_COEF_SEED[ind])
        for S in (1, 64, 1024):
            src = synth.source(seed + S, 0, F, k, S)
            shaped = (lambda x: x[:, :, 0]) if S == 1 else (lambda x: x)
            if triangle:     # the encoder produces the codewords: S = 1 the serial kernel's one sweep, packets the static schedule of up to m levels
                cw = ctx.encode(h, shaped(src))
                for f in range(F):
                    assert np.array_equal(cw[f].reshape(n, S), oc.encode(src[f]).reshape(n, S)), (name, S, f)
            else:            # no systematic encoder (refused): codewords by the reference's own sweeps
                with pytest.raises(api.LdpcAmdError):
                    ctx.encode(h, shaped(src))
                cw = shaped(np.stack([rm.codeword_by_sweeps(oc, code, src[f]) for f in range(F)]))
                assert not rm.syndrome(code, cw[0]).any()
            sym = np.ascontiguousarray(cw).copy()
            sym[era.astype(bool)] = 0x77
            sym = rm.corrupt(rng, sym, era)
            for sweeps in caps:
                fits = rm.fits(m, sweeps)
                for do_ml in (1, 0):
                    exp = _oracle_frames(oc, sym, era, S, sweeps, do_ml)
                    seen |= {e[4] for e in exp}
                    for knobs in _knob_sets(S):
                        what = (name, S, sweeps, do_ml, tuple(knobs.values()))
                        ctx.configure_many(knobs)
                        try:
                            ctx.configure("PEEL_RELAX", "1")
                            a = ctx.decode(h, sym, era, max_sweeps=sweeps, do_ml=do_ml)
                            used = ctx.profile_kernel_names()["peel"]
                            ctx.configure("PEEL_RELAX", "0")
                            b = ctx.decode(h, sym, era, max_sweeps=sweeps, do_ml=do_ml)
                            serial = ctx.profile_kernel_names()["peel"]
                        finally:
                            ctx.configure("PEEL_RELAX", None)
                            ctx.configure_many({kk: None for kk in knobs})
                        assert ("relax" in used) == fits, (what, used)     # the fall-back is taken exactly when the keys do not fit
                        assert "relax" not in serial, (what, serial)
                        for x, y, w in zip(a, b, WHAT):
                            assert np.array_equal(x, y), (what, w)
                        _equals_the_oracle(a, exp, sym, era, S, what)
    if name.startswith("staircase_m") and m >= 320:
        assert seen == {0, 1, 2, 3}, (name, seen)     # sweeps done, ML solved, ML rank deficient, ML not run
