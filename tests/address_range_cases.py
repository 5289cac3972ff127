"""The small problems behind tests/test_address_range_cpu.py and tests/test_gpu_address_range.py: P = 4080 byte lanes (or PF = 7
frames), every expected byte and status word from the CPU oracle.  The GPU test tiles them up to the sizes at the edges of the
kernels' address range (tools/address_range.py); the CPU test shows on the oracle alone that tiling is sound and that the erasure
patterns chosen here give the status classes the GPU test relies on.  Computed once per process, shared, read-only."""
import os
import sys

import numpy as np

from code_helpers import random_code
from ldpc_erasure_codes_amd import api, codes, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import address_range as ar  # noqa: E402

P, PF = ar.P, ar.PF
_CACHE = {}


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, tuple):
            for x in v:
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)
    return d


def get_code(which):
    """(codes.Code, OracleCode): a built-in code by index, or the light-column triangle codes "r300" (300,200), "r64" (64,44) and
    "r3" (3,1: two chained checks, the smallest code whose encoder has the persistent packet-output form) that code_helpers.random_code builds."""
    key = ("code", which)
    if key not in _CACHE:
        from oracle import oracle_py
        if which == "r300":
            code = random_code()
        elif which == "r64":
            code = random_code(n=64, k=44, coldeg=3, seed=5)
        elif which == "r3":
            code = random_code(n=3, k=1, coldeg=1, seed=7)
        else:
            code = codes.load_builtin(which)
        _CACHE[key] = (code, oracle_py.OracleCode(code))
    return _CACHE[key]


def oracle_decode(oc, sym, era, do_ml=1, it=10):
    """(out, sweeps, residual, status) of every frame from the oracle alone (status depends on the pattern only)."""
    F, n, S = sym.shape
    out = np.zeros_like(sym)
    _, sw, res, st = oc.decode_batch_s1(np.zeros((F, n), dtype=np.uint8), era, itenum=it, do_ml=do_ml)
    for f in range(F):
        out[f], _, it_f, info, _ = oc.decode_packets(sym[f], era[f], itenum=it, do_ml=do_ml)
        assert it_f == sw[f] and info[0] == res[f]
    return out, sw.astype(np.int32), res.astype(np.int32), st.astype(np.int32)


def received(cw, era, noncodeword, seed):
    """The received frames: erased payloads are 0xA5 (ignored); in the frames listed in `noncodeword` one received source row
    is replaced by noise, in every lane."""
    sym = cw.copy()
    sym[era.astype(bool)] = 0xA5
    rng = np.random.default_rng(seed)
    for f in noncodeword:
        j = int(np.nonzero(era[f] == 0)[0][min(3, int((era[f] == 0).sum()) - 1)])
        sym[f, j] = rng.integers(0, 256, sym.shape[2], dtype=np.uint8)
    return sym


def light_case(which, lanes=P):
    """F = 2 frames of a light-column code at `lanes` byte lanes: frame 0 a codeword with about 8 % erasures, frame 1 a
    non-codeword with about 5 %.  Source, oracle codewords, received frames, the oracle's decode."""
    key = ("light", which, lanes)
    if key not in _CACHE:
        code, oc = get_code(which)
        rng = np.random.default_rng(11 + code.n)
        era = np.stack([(rng.random(code.n) < p).astype(np.uint8) for p in (0.08, 0.05)])
        if not era[0].any():
            era[0, code.n - 1] = 1                              # (a tiny code: at least the last parity symbol)
        src = rng.integers(0, 256, (2, code.k, lanes), dtype=np.uint8)
        cw = np.stack([oc.encode(src[f]) for f in range(2)])
        sym = received(cw, era, (1,), 5)
        want = oracle_decode(oc, sym, era)
        assert int(era[0].sum()) - int(want[2][0]) >= 1          # frame 0 has steps to run
        _CACHE[key] = _frozen(dict(code=code, era=era, src=src, cw=cw, sym=sym, want=want))
    return _CACHE[key]


# ---- the built-in (2040,1530) code: one pattern per status class ---------------------------------------------------------
B_CODE = 1
B_LOW, B_HIGH = 150, 400      # steps of the "few steps" / "many steps" frames: either side of any tier-1 capacity between them
B_CLASSES = ("lo", "hi", "ml1", "ml2")


def b_patterns():
    """{class: erasure pattern [n]} chosen on the oracle: lo / hi = message passing completes (status 0) in at most B_LOW / at
    least B_HIGH steps, ml1 = the ML stage solves (status 1), ml2 = rank deficient (status 2).  Without the ML stage (do_ml = 0)
    ml1 and ml2 are status 3."""
    key = "b_patterns"
    if key not in _CACHE:
        code, oc = get_code(B_CODE)
        found = {}
        for p, seed in ((0.05, 3), (0.19, 4), (0.20, 5), (0.21, 6), (0.235, 7), (0.27, 8)):
            era = synth.erasures_uniform(seed, 0, 48, code.n, p)
            _, _, res, st = oc.decode_batch_s1(np.zeros_like(era), era)
            steps = era.sum(1) - res
            for f in range(era.shape[0]):
                cls = None
                if st[f] == 0 and steps[f] <= B_LOW:
                    cls = "lo"
                elif st[f] == 0 and steps[f] >= B_HIGH:
                    cls = "hi"
                elif st[f] == 1:
                    cls = "ml1"
                elif st[f] == 2:
                    cls = "ml2"
                if cls and cls not in found:
                    found[cls] = era[f].copy()
        assert set(found) == set(B_CLASSES), sorted(found)
        _CACHE[key] = _frozen(found)
    return _CACHE[key]


# the frames of the small (2040,1530) problem; "nc" = the ml1 pattern on a non-codeword
B_FRAMES = ("lo", "hi", "ml1", "ml2", "nc")
# the GPU test's runs of F = 3 (frame 1 starts beyond 2^32 bytes, frame 2 beyond 2^33): (frames, do_ml)
B_RUNS = ((("lo", "hi", "ml1"), 1), (("ml2", "nc", "hi"), 1), (("hi", "ml2", "ml1"), 0))


def b_case(lanes=P):
    key = ("b", lanes)
    if key not in _CACHE:
        code, oc = get_code(B_CODE)
        pat = b_patterns()
        era = np.stack([pat["ml1" if c == "nc" else c] for c in B_FRAMES])
        F = era.shape[0]
        src = synth.source(77, 0, F, code.k, lanes)
        cw = np.stack([oc.encode(src[f]) for f in range(F)])
        sym = received(cw, era, (B_FRAMES.index("nc"),), 9)
        want = {ml: oracle_decode(oc, sym, era, do_ml=ml) for ml in (1, 0)}
        _CACHE[key] = _frozen(dict(code=code, era=era, src=src, cw=cw, sym=sym, want1=want[1], want0=want[0]))
    return _CACHE[key]


def b_run(c, frames, do_ml):
    """The rows of b_case() a run uses: (sym, era, (out, sweeps, residual, status))."""
    idx = [B_FRAMES.index(x) for x in frames]
    want = c["want1" if do_ml else "want0"]
    return c["sym"][idx], c["era"][idx], tuple(w[idx] for w in want)


# ---- the batch axis: PF frames of the (2040,1530) code --------------------------------------------------------------------
def batch_case(S):
    """PF = 7 frames at S = 1 or a packet length: 10 % erasures, frame 5 with 21 % (beyond message passing), frame 3 a
    non-codeword."""
    key = ("batch", S)
    if key not in _CACHE:
        code, oc = get_code(B_CODE)
        era = synth.erasures_uniform(21, 0, PF, code.n, 0.10)
        era[5] = b_patterns()["ml1"]
        src = synth.source(78, 0, PF, code.k, S)
        cw = np.stack([oc.encode(src[f]) for f in range(PF)])
        sym = received(cw, era, (3,), 10)
        if S == 1:
            out, sw, res, st = oc.decode_batch_s1(sym[:, :, 0], era)
            want = (out, sw.astype(np.int32), res.astype(np.int32), st.astype(np.int32))
            d = dict(code=code, era=era, src=src[:, :, 0].copy(), cw=cw[:, :, 0].copy(), sym=sym[:, :, 0].copy(), want=want)
        else:
            d = dict(code=code, era=era, src=src, cw=cw, sym=sym, want=oracle_decode(oc, sym, era))
        assert 1 in d["want"][3].tolist() and 0 in d["want"][3].tolist()
        _CACHE[key] = _frozen(d)
    return _CACHE[key]


# ---- Reed-Solomon (255,223) -----------------------------------------------------------------------------------------------
RS_N, RS_K = 255, 223


def rs_case(lanes=P):
    """B = 2 blocks.  Gathered rows: block 0 misses r = 32 source symbols (every repair symbol needed), block 1 misses 5.
    Frames: block 0 the same (erasure flags), block 1 short (k - 3 received: zeros, RS_ST_SHORT).  Every lane through the oracle."""
    key = ("rs", lanes)
    if key not in _CACHE:
        from oracle import oracle_py
        n, k = RS_N, RS_K
        rng = np.random.default_rng(31)
        g = oracle_py.rs_generator(n, k)
        src = rng.integers(0, 256, (2, k, lanes), dtype=np.uint8)
        cw = np.zeros((2, n, lanes), dtype=np.uint8)
        for b in range(2):
            for s in range(lanes):
                cw[b, :, s] = oracle_py.rs_encode(g, np.ascontiguousarray(src[b, :, s]))
        era = np.zeros((2, n), dtype=np.uint8)
        era[0, rng.choice(k, n - k, replace=False)] = 1
        era[1, rng.choice(k, 5, replace=False)] = 1
        idx = np.stack([np.nonzero(era[b] == 0)[0][:k] for b in range(2)]).astype(np.uint16)
        assert int((idx[0] >= k).sum()) == n - k
        val = np.stack([cw[b, idx[b]] for b in range(2)])
        msg = np.zeros((2, k, lanes), dtype=np.uint8)
        for b in range(2):
            for s in range(lanes):
                m, rc = oracle_py.rs_decode(g, idx[b], np.ascontiguousarray(val[b, :, s]))
                assert rc == 0
                msg[b, :, s] = m
        # frames: block 1 short
        fera = era.copy()
        fera[1] = 0
        fera[1, rng.choice(n, n - k + 3, replace=False)] = 1
        fsym = cw.copy()
        fsym[fera.astype(bool)] = 0x5A
        fmsg = msg.copy()
        fmsg[1] = 0
        _CACHE[key] = _frozen(dict(g=g, src=src, cw=cw, idx=idx, val=val, msg=msg, fera=fera, fsym=fsym, fmsg=fmsg,
                                   received=(1 - fera).sum(1).astype(np.int32),
                                   status=np.array([api.RS_ST_DECODED, api.RS_ST_SHORT], dtype=np.int32)))
    return _CACHE[key]
