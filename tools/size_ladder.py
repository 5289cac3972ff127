#!/usr/bin/env python3
"""The size ladder: registered codes that straddle the size switches of the launch plans, one small batch of frames per code.

`ldpc_amd_register_code` takes any n <= 65534 and row degree <= 24; which kernels then run is decided on the host from n, m, the
degree pad and max_sweeps (csrc/kernels.hip: plan_peel, plan_relax, plan_scatter, plan_encode, plan_ml).  Every RUNG below is a code
named for the switch it sits on ("Code sizes").  tests/test_size_ladder_cpu.py pins the ladder on the oracle;
tests/test_gpu_size_ladder.py takes it through the C ABI.

Codes.  All are built straight as CSR (a dense H at n = 65534 is gigabytes) and are in triangle form: check r ends at its own
parity column k + r, so encode, decode and the oracle all apply.  tools/relax_model.py's `random_triangle_code` picks a check's
earlier parity columns uniformly, which makes the first parity columns heavy (about 2 ln m entries: more than 16 from m = 2048 on)
and would send every large rung to the gather kernel; `ladder_code` keeps every column at 16 entries or fewer instead: the source
columns are dealt round robin from shuffled decks, a check takes the parity column before it (probability 0.8, the chain) and one
from the 64 before that.  Three small planted structures in the LAST source columns make the frame kinds a matter of construction,
not of luck:
  k-8 .. k-5   G: four columns that are in four checks and in no other -- erased together, the sweeps stall on a 4 x 4 system
               that the ML stage solves (square: its solution is unique whatever the received symbols are)
  k-4 .. k-2   H: a chain AGAINST the sweep order.  Checks c3 < c2 < c1: c1 holds h1; c2 holds h1, h2; c3 holds h2, h3.  Erased
               together they take exactly three sweeps (with max_sweeps = 1 two are left, a full-rank residual)
  k-1          Z: a column in no check.  Erased, it can never be recovered: residual 1, rank deficient (status 2)

Batches (`batch(rung)`): at most 9 frames -- the five chosen step counts below, which no smaller batch holds beside the other kinds:
  none         no erasure: the codeword must come back as it went in
  t<T>         parity only, exactly T steps in one sweep (tools/step_patterns.parity_subset): T on both sides of 2 * 256 and
               2 * 512 (the steps a 256- / 512-thread packet kernel holds in registers) and T = m; in the T = 513 frame two received symbols are
               changed: it is no codeword
  sweeps3      H + 64 parity symbols: message passing completes in three sweeps
  ml           G + 64 parity symbols: the ML stage solves it
  deficient    Z + 32 parity symbols (status 2), or -- `all` -- every symbol that is in a check (E > m: skipped, status 3)
Erasure flags take the values 1, 2, 0x80 and 0xFF ("non-zero = erased", include/ldpc_erasure_amd.h); `flags01` is the same batch
normalised, from which every expectation is computed.

`host_plan` mirrors the host arithmetic of csrc/kernels.hip in a few lines -- what is refused and why, which peel kernel runs, the
packet plan -- so that the refused list of the GPU test can be checked by hand.  numpy and the package's host side only."""
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ldpc_erasure_codes_amd import codes  # noqa: E402
from relax_model import is_triangle  # noqa: E402
from step_patterns import parity_subset  # noqa: E402

FLAG_VALUES = (1, 2, 0x80, 0xFF)
PLANTED = 8            # source columns the planted structures take (the last ones)
STEP_COUNTS = (2 * 256 - 1, 2 * 256 + 1, 2 * 512 - 1, 2 * 512 + 1)


# ---- the rungs: name -> (n, m, largest row degree, sweep caps the GPU test runs) ---------------------------------------------------
@dataclass(frozen=True)
class Rung:
    name: str
    n: int
    m: int
    deg: int                      # entries per check: deg - 1 or deg
    sweeps: tuple = (10,)         # max_sweeps values: (1, 3, 10) where they move plan_relax's keys_fit
    switch: str = ""
    band: int = 0                 # > 0: that many earlier parity columns per check (see ladder_code), not two

    @property
    def k(self):
        return self.n - self.m


RUNGS = (
    Rung("n2048_m512", 2048, 512, 8, switch="the foot of the ladder: all m accumulators fit at 256-byte pieces, two tiers"),
    Rung("n4000_m1984", 4000, 1984, 8, switch="plan_scatter halves B twice: 64-byte pieces, two tiers off because of size"),
    Rung("n4096_m1024", 4096, 1024, 8, switch="relaxation: last n with 64-bit flag loads; packet kernel: last n its 1024 threads hold in registers"),
    Rung("n4099_m1025", 4099, 1025, 8, switch="n odd: the byte paths of every flag and output loop"),
    Rung("n4104_m1026", 4104, 1026, 8, switch="relaxation: first n % 8 == 0 past the 64-bit flag loads; the loop behind the 1024-thread set-up"),
    Rung("n8192_m4096_d8", 8192, 4096, 8, switch="packet kernel at 16-byte pieces (256 threads) with m at the ML limit"),
    Rung("n8192_m4096_d14", 8192, 4096, 14, switch="serial peel's LDS plan does not fit, the relaxation's does (tables from global memory)"),
    Rung("n8208_m4097_d8", 8208, 4097, 8, (1, 3, 10), "first m the ML stage refuses; logM 13: keys fit at max_sweeps 3, not at 10"),
    Rung("n11008_m5504_d16", 11008, 5504, 16, (3, 10), "13 earlier parity columns per check: 70 000 entries in the encoder's compact lists of the parity symbols, "
         "past their 16-bit offsets -- dropped at registration, scatter encoder without them; degree pad 16", band=13),
    Rung("n16392_m8193_d8", 16392, 8193, 8, (1, 3, 10), "logM 14: keys fit at max_sweeps 1 only; no packet plan: gather kernel"),
    Rung("n32760_m2048_d8", 32760, 2048, 8, switch="relaxation: n % 8 == 0 below its n limit"),
    Rung("n32767_m2047_d8", 32767, 2047, 8, switch="relaxation: its largest n; rx_off = 2 * col still fits 16 bits"),
    Rung("n32768_m2048_d8", 32768, 2048, 8, switch="first n past the relaxation: rx_off wraps, the serial peel must run"),
    Rung("n49152_m4096_d8", 49152, 4096, 8, switch="between the relaxation's limit and the registration limit"),
    Rung("n65534_m1024_d8", 65534, 1024, 8, switch="registration limit: row index 65533 beside the 0xFFFF sentinels"),
    Rung("n65534_m16384_d8", 65534, 16384, 8, (1, 10), "no decoder plan holds the code; the encoder's gather kernel with 98 KB of LDS"),
    Rung("n65534_m27307_d8", 65534, 27307, 8, switch="first m whose gather tables (6 m + 4 bytes) pass 160 KB: refused on every path"),
)
BY_NAME = {r.name: r for r in RUNGS}


# ---- codes ------------------------------------------------------------------------------------------------------------------------
def ladder_code(rung):
    """codes.Code of the rung (see the module docstring); also returns the planted structure: dict G / H / Z -> columns, and the
    checks that hold them."""
    n, m, k, deg = rung.n, rung.m, rung.k, rung.deg
    rng = np.random.default_rng([77, n, m, deg])
    free = k - PLANTED                                     # source columns dealt round robin
    G = list(range(k - 8, k - 4))
    H = list(range(k - 4, k - 1))
    Z = k - 1
    g_checks = sorted(int(x) for x in (m // 7, m // 3, m // 2 + 1, m - 5))
    c3, c2, c1 = m // 5, m // 5 + 70, m - 9               # c3 < c2 < c1, in different chunks of 64 checks
    planted = {c: list(G) for c in g_checks}
    planted.setdefault(c1, []).append(H[0])
    planted.setdefault(c2, []).extend([H[0], H[1]])
    planted.setdefault(c3, []).extend([H[1], H[2]])
    assert len({c1, c2, c3} | set(g_checks)) == 7

    deck = np.empty(0, dtype=np.int64)
    pos = 0
    row_ptr, cols = [0], []
    for r in range(m):
        want = deg if rng.random() < 0.8 else deg - 1
        par = []
        extra = planted.get(r, [])
        if rung.band:
            # parity columns r - 65 - 5 j: none from the check's own chunk of 64 (the relaxation settles such a chunk in one pass), and
            # column c is in checks c + 65 + 5 j only -- band + 1 entries per parity column
            want = deg
            par = [k + r - 65 - 5 * j for j in range(rung.band) if r - 65 - 5 * j >= 0][:deg - 1 - len(extra)]
        else:
            if r >= 2:
                par.append(k + r - int(rng.integers(2, min(r, 64) + 1)))
            if r >= 1 and want == deg:
                par.append(k + r - 1)
        nsrc = max(0, want - 1 - len(par) - len(extra))
        if pos + nsrc > deck.size:
            deck = np.concatenate([deck[pos:], rng.permutation(free), rng.permutation(free)])
            pos = 0
        src = set()
        while len(src) < nsrc:                             # (a deck boundary can deal a column twice: take the next card)
            src.add(int(deck[pos]))
            pos += 1
            if pos >= deck.size:
                deck = rng.permutation(free)
                pos = 0
        cols += sorted(src) + sorted(extra) + sorted(par) + [k + r]
        row_ptr.append(len(cols))
    coefs = rng.integers(1, 256, size=len(cols)).astype(np.uint8)
    code = codes.Code(n, k, np.array(row_ptr, dtype=np.uint32), np.array(cols, dtype=np.uint16), coefs, rung.name)
    return code, {"G": G, "H": H, "Z": Z, "g_checks": g_checks, "h_checks": (c3, c2, c1)}


def code_facts(code):
    rp = code.row_ptr.astype(np.int64)
    deg = np.diff(rp)
    coldeg = np.bincount(code.cols.astype(np.int64), minlength=code.n)
    # entries of the encoder's compact lists (api.cpp: enc_lst): the lists of the PARITY symbols without each one's own check
    return {"triangle": is_triangle(code), "maxdeg": int(deg.max()), "mindeg": int(deg.min()), "maxcoldeg": int(coldeg.max()),
            "enc_lst": int((code.cols.astype(np.int64) >= code.k).sum()) - code.m,
            "nnz": int(rp[-1]), "ascending": all(np.all(np.diff(code.cols[rp[r]:rp[r + 1]].astype(np.int64)) > 0) for r in range(code.m)),
            "uncovered": int((coldeg == 0).sum())}


# ---- batches ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Batch:
    kinds: list                    # one name per frame
    steps: list                    # chosen step count of a parity-only frame, else None
    flags: np.ndarray              # uint8 [F, n]: 0 or one of FLAG_VALUES
    corrupt: list                  # (frame, symbol, xor value): received symbols changed behind the encoder
    planted: dict = field(default_factory=dict)

    @property
    def flags01(self):
        return (self.flags != 0).astype(np.uint8)


def batch(rung, code=None, planted=None):
    if code is None:
        code, planted = ladder_code(rung)
    n, m, k = code.n, code.m, code.k
    rng = np.random.default_rng([78, n, m])
    kinds, steps, rows, corrupt = [], [], [], []

    def add(kind, fl, t=None):
        kinds.append(kind); steps.append(t); rows.append(fl)

    def parity_but(t, avoid):
        """t parity symbols, none of them the own column of a check in `avoid` (the planted checks keep their equations whole)"""
        ok = np.setdiff1d(np.arange(m), np.asarray(sorted(avoid)))
        fl = np.zeros(n, dtype=np.uint8)
        fl[k + rng.choice(ok, size=min(t, ok.size), replace=False)] = 1
        return fl

    add("none", np.zeros(n, dtype=np.uint8))
    for t in sorted({min(t, m) for t in STEP_COUNTS} | {m}):
        add("t%d" % t, parity_subset(code, t, 100 + t, "random"), t)
    fl = parity_but(64, set(planted["h_checks"]))
    fl[planted["H"]] = 1
    add("sweeps3", fl)
    fl = parity_but(64, set(planted["g_checks"]))
    fl[planted["G"]] = 1
    add("ml", fl)
    if RUNGS.index(rung) % 3 != 1:                         # (both forms appear on the ladder)
        fl = parity_but(32, set())
        fl[planted["Z"]] = 1
        add("deficient", fl)
    else:
        fl = np.zeros(n, dtype=np.uint8)
        fl[np.unique(code.cols.astype(np.int64))] = 1
        add("all", fl)
    flags = np.stack(rows)
    # every non-zero value, spread so that neighbouring symbols (the bytes of one 64-bit flag load) differ
    vals = np.array(FLAG_VALUES, dtype=np.uint8)[(np.arange(n)[None, :] * 3 + np.arange(flags.shape[0])[:, None]) % 4]
    flags = np.where(flags != 0, vals, 0).astype(np.uint8)
    for f in (kinds.index("t513") if "t513" in kinds else kinds.index("t511"),):
        known = np.flatnonzero(flags[f] == 0)
        for j in rng.choice(known, size=2, replace=False):
            corrupt.append((f, int(j), 0x21))
    return Batch(kinds, steps, flags, corrupt, planted)


def source(rung, S, F):
    """uint8 [F, k, S] source symbols of the rung's batch."""
    return np.random.default_rng([79, rung.n, rung.m, S]).integers(0, 256, size=(F, rung.k, S), dtype=np.uint8)


def received(cw, b):
    """The batch's received symbols from its codewords [F, n, S]: the changed symbols changed, the erased ones overwritten."""
    sym = np.array(cw, dtype=np.uint8, copy=True)
    for f, j, x in b.corrupt:
        sym[f, j] ^= x
    sym[b.flags != 0] = 0xEE
    return sym


# ---- the host arithmetic of csrc/kernels.hip ---------------------------------------------------------------------------------------
LDS_MAX = 160 * 1024


def _au(v, a=16):
    return (v + a - 1) // a * a


def _peel_lds(n, m, mpad, degpad, fused, gt):
    off = 0 if gt else _au(degpad * mpad * (4 if fused else 2))
    off += 768 if fused else 0
    w = max(_au(2 * n), _au(4 * (m + 2)) + _au(4 * m)) + _au(max(4 * m, n if fused else 0)) + _au(2 * m)
    return off + w


def _relax_lds(n, m, mpad, degpad, mode, gt):
    off = 0 if gt else _au(2 * degpad * mpad) + (_au(degpad * mpad) if mode == 0 else 0)
    off += 768
    w = _au(2 * (n + 1)) + 2 * _au(2 * mpad)
    w += 256 if mode != 2 else _au(max(4 * (m + 2), 256)) + 2 * _au(mpad)
    return off + w


def _ml_lds(n, m, mpad):
    off = _au(max(12 * m, 4 * m + 2 * n, 4 * (2 * m + 4) + 2 * m + 16)) + _au(2 * m) + _au(3 * mpad) + _au(2 * m + 2) + 2 * _au(2 * m)
    return off + _au(m) + 8192 + 256 + 1024 + 128 + 4 * 16 + _au(4 * (m + 2))


def _scatter(n, m, S):
    """bytes of every row per workgroup (0: no plan), two tiers"""
    B = 256
    while B > 16 and S % B:
        B >>= 1
    tail = _au(2 * m) + _au(m) + _au(2 * (m + 2)) + 288 + _au(2 * n) + _au(2 * (m + 2)) + 8192
    while B > 16 and m * B + tail > 156 * 1024:
        B >>= 1
    if m * B + tail > LDS_MAX:
        return 0, False
    tcap = (LDS_MAX // 2 - tail) // B
    return B, (B >= 128 and m // 4 <= tcap < m)


def host_plan(n, m, maxdeg, maxcoldeg, entry, S, max_sweeps=10, do_ml=1):
    """What the host decides for one call.  entry: "encode", "decode", "decode_frames" or "inplace".  Returns a dict:
    refused (None or the start of the error text), peel ("relax" | "serial" | None), tables_in_global, packet_bytes, two_tiers,
    gather.  Default knobs."""
    mpad = _au(m, 64)
    degpad = 8 if maxdeg <= 8 else (14 if maxdeg <= 14 else (16 if maxdeg <= 16 else 24))
    p = {"refused": None, "peel": None, "tables_in_global": False, "packet_bytes": 0, "two_tiers": False, "gather": False,
         "why_serial": None}
    fused = S == 1
    if entry == "encode":
        if fused:                                           # one in-order sweep of the serial kernel, no flags
            need = _peel_lds(n, m, mpad, degpad, True, False)
            if need > LDS_MAX and _peel_lds(n, m, mpad, degpad, True, True) > LDS_MAX:
                p["refused"] = "code too large for LDS"
            p["peel"], p["tables_in_global"] = "serial", need > LDS_MAX
            return p
        B = _scatter(n, m, S)[0] if maxcoldeg <= 16 else 0
        p["packet_bytes"], p["gather"] = B, B == 0
        if B == 0 and 6 * m + 4 > LDS_MAX:
            p["refused"] = "gather kernel: LDS need"
        return p
    B, two = (_scatter(n, m, S) if (not fused and maxcoldeg <= 16) else (0, False))
    p["packet_bytes"], p["two_tiers"], p["gather"] = B, two, (not fused and B == 0)
    if entry == "inplace" and B == 0:
        p["refused"] = "in-place decode needs the scatter kernel"
        return p
    logM = 0
    while (1 << logM) < mpad:
        logM += 1
    mode = 0 if fused else 2
    keys = degpad <= 16 and n <= 32767 and max_sweeps <= 62 and ((max_sweeps + 1) << logM) <= 65535
    fits_l = _relax_lds(n, m, mpad, degpad, mode, False) <= LDS_MAX
    fits_g = _relax_lds(n, m, mpad, degpad, mode, True) <= LDS_MAX
    if keys and (fits_l or fits_g):
        p["peel"], p["tables_in_global"] = "relax", not fits_l
    else:
        p["peel"] = "serial"
        p["why_serial"] = "n" if n > 32767 else ("keys" if not keys else "lds")
        need = _peel_lds(n, m, mpad, degpad, fused, False)
        if need > LDS_MAX and (not fused or _peel_lds(n, m, mpad, degpad, True, True) > LDS_MAX):
            p["refused"] = "code too large for LDS"
            return p
        p["tables_in_global"] = need > LDS_MAX
    if p["gather"] and 6 * m + 4 > LDS_MAX:
        p["refused"] = "gather kernel: LDS need"
    elif do_ml and _ml_lds(n, m, mpad) > LDS_MAX:
        p["refused"] = "ML stage: LDS need"
    elif do_ml and m > 4096:
        p["refused"] = "ML stage: more than 4096 checks"
    elif do_ml and _ml_lds(n, m, mpad) + 256 > LDS_MAX:    # (plan_ml: the matrix wants 256 bytes behind the tables)
        p["refused"] = "ML stage: LDS need"
    return p


if __name__ == "__main__":
    import time
    for rung_ in RUNGS:
        t0_ = time.time()
        code_, planted_ = ladder_code(rung_)
        b_ = batch(rung_, code_, planted_)
        facts_ = code_facts(code_)
        print("%-18s %5.2f s  deg %d..%d  coldeg %d  nnz %d  frames %s" % (rung_.name, time.time() - t0_, facts_["mindeg"], facts_["maxdeg"],
                                                                           facts_["maxcoldeg"], facts_["nnz"], ",".join(b_.kinds)))
        for entry_ in ("encode", "decode", "inplace"):
            for S_ in (1, 16, 256):
                if entry_ == "inplace" and S_ == 1:
                    continue
                for ms_ in rung_.sweeps:
                    for ml_ in ((0,) if entry_ == "encode" else (0, 1)):
                        p_ = host_plan(rung_.n, rung_.m, facts_["maxdeg"], facts_["maxcoldeg"], entry_, S_, ms_, ml_)
                        print("    %-8s S %3d sweeps %2d ml %d  %s" % (entry_, S_, ms_, ml_, {k_: v_ for k_, v_ in p_.items() if v_}))
                    if entry_ == "encode":
                        break
