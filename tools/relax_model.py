#!/usr/bin/env python3
"""CPU model of the exact time-stamp relaxation (csrc/peel_relax.inc), its evaluation loop in executable form, and the
chain-structured code families that stress it.

The reference sweeps the checks in order and solves a check's last erased neighbour at once
(Matlab/My_LDPC_HybridML_NonBinary_Erasure_Decoder.m:21-59).  The kernel instead keeps one 16-bit KEY per symbol -- the visit
(sweep << logM | check) at which it is resolved, kKnown for a received symbol, kInf for "never" -- and evaluates chunks of 64
checks round robin: every check reads the keys of its neighbours, takes the top two, proposes next_visit(check, second key)
to its latest neighbour, and the smallest proposal wins.  All 64 checks of a chunk read BEFORE any of them writes, so a
dependency between two checks of one chunk costs a whole round-robin pass: a staircase (dual-diagonal) parity part needs
about m passes where the reference needs one sweep.

`relax` replays that loop (peel_relax.inc:204-299: one evaluation per visit, stop after `nch` clean evaluations in a row) and
counts the evaluations; `eval_budget` mirrors the kernel's safety cap.  tests/test_relax_model_cpu.py pins the model's fixed
point on the oracle's sequential sweep and checks evaluations <= eval_budget for the families below; the GPU tests
(tests/test_gpu_relax_structured.py) take the same codes and erasure patterns through the kernels.  Test infrastructure, not
product code."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pi_model import INV, MUL  # noqa: E402  (GF(256) tables of the project's field)

from ldpc_erasure_codes_amd import codes  # noqa: E402

K_INF = 0xFFFF
CHUNK = 64          # checks per evaluation: one per lane of a wavefront
MAX_SWEEPS = 62     # the time sort's 64 per-sweep counters (peel_relax.inc:379-398)
MAX_DEG = 16        # 4-bit neighbour slot of the top-2 key


# ---- the kernel's limits ----------------------------------------------------------------------------------------------------------
def log_m(m):
    """logM of plan_relax (kernels.hip: `while ((1 << r.logM) < cd.mpad) r.logM++`)."""
    mpad = -(-m // CHUNK) * CHUNK
    lg = 0
    while (1 << lg) < mpad:
        lg += 1
    return lg


def fits(m, max_sweeps):
    """The sweep-cap half of plan_relax's `keys_fit` (kernels.hip): the keys fit 16 bits and the sweeps fit the time sort's counters."""
    return max_sweeps <= MAX_SWEEPS and ((max_sweeps + 1) << log_m(m)) <= 65535


def largest_fitting_sweeps(m):
    return min(MAX_SWEEPS, 65535 // (1 << log_m(m)) - 1)


def eval_budget(nch, m, max_sweeps):
    """Evaluations the kernel allows itself before it reports kDevErrRelaxCap.
    Mirrors `long budget = (long)nch * ((long)m + 2)` in csrc/peel_relax.inc (the safety cap in front of the relaxation loop).
    Any nch evaluations in a row visit every chunk once and settle at least the earliest key that is still wrong; at most m keys
    are ever written (a check solves at most one symbol), and the loop then needs nch clean evaluations: nch * (m + 1) in all.
    `max_sweeps` does not enter: a long chain is resolved inside ONE sweep."""
    return nch * (m + 2)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def neighbour_table(code):
    """[mpad, degpad] symbol of every neighbour slot in CSR order, padding slots and padding rows = n (DevCode::rx_off / 2)."""
    m, n = code.m, code.n
    mpad = -(-m // CHUNK) * CHUNK
    rp = code.row_ptr.astype(np.int64)
    deg = int(np.diff(rp).max())
    if deg > MAX_DEG:
        raise ValueError("row degree %d: the relaxation takes at most %d neighbours" % (deg, MAX_DEG))
    degpad = 8 if deg <= 8 else (14 if deg <= 14 else 16)
    nbr = np.full((mpad, degpad), n, dtype=np.int64)
    coef = np.zeros((mpad, degpad), dtype=np.uint8)
    for r in range(m):
        s, e = int(rp[r]), int(rp[r + 1])
        nbr[r, :e - s] = code.cols[s:e]
        coef[r, :e - s] = code.coefs[s:e]
    return nbr, coef


class Tables:
    """Per-code tables of the model, built once and shared by the frames."""

    def __init__(self, code):
        self.code = code
        self.n, self.m = code.n, code.m
        self.nbr, self.coef = neighbour_table(code)
        self.mpad, self.degpad = self.nbr.shape
        self.nch = self.mpad // CHUNK
        self.logM = log_m(self.m)
        # chunks that read a symbol's key (for the exact short cut of `relax`)
        self.readers = [[] for _ in range(self.n + 1)]
        for c in range(self.nch):
            for j in np.unique(self.nbr[c * CHUNK:(c + 1) * CHUNK]):
                self.readers[int(j)].append(c)


def relax(tab, erased, max_sweeps, skip_unchanged=True, budget=None):
    """One frame through the relaxation loop.  erased: [n] flags.  Returns a dict:
         keys         int [n]   final time stamps (kKnown: received, K_INF: never resolved)
         pairs        list of (check, symbol) in time order: the solving checks at the fixed point
         iterations   the reference's `iterations` (:130)
         residual     sorted symbols still unknown
         evaluations  chunk evaluations the kernel's loop performs, the final clean round included
         capped       True if `budget` evaluations did not reach the fixed point (the kernel would report kDevErrRelaxCap)
    skip_unchanged: a chunk none of whose input keys changed since its last evaluation would compute what it computed then -- no
    improvement, the same solver marks -- so it is counted without being computed.  Exact; False replays every evaluation."""
    n, m, nch, logM = tab.n, tab.m, tab.nch, tab.logM
    if not fits(m, max_sweeps):
        raise ValueError("max_sweeps = %d: the keys of m = %d do not fit (the host takes the serial kernel)" % (max_sweeps, m))
    k_known = (1 << logM) - 1
    erased = np.asarray(erased).astype(bool)
    key = np.where(erased, K_INF, k_known).astype(np.int64)
    key = np.append(key, k_known)                     # the padding neighbour
    fire = np.full(tab.mpad, -1, dtype=np.int64)      # symbol the check solves, -1: none
    slot_id = np.arange(tab.degpad, dtype=np.int64)
    lane = np.arange(CHUNK, dtype=np.int64)
    evaluations, capped = 0, False
    if erased.any():
        dirty = np.ones(nch, dtype=bool)
        clean, ch = 0, 0
        while clean < nch:
            if skip_unchanged and not dirty[ch]:
                # run of unchanged chunks up to the next changed one (or to the end of the clean round)
                ahead = np.flatnonzero(np.roll(dirty, -ch))
                run = min(int(ahead[0]) if ahead.size else nch, nch - clean)
                if budget is not None and evaluations + run > budget:
                    evaluations, capped = budget, True
                    break
                evaluations += run
                clean += run
                ch = (ch + run) % nch
                continue
            if budget is not None and evaluations >= budget:
                capped = True
                break
            evaluations += 1
            rows = ch * CHUNK + lane
            nb = tab.nbr[rows]
            v = (key[nb] << 4) | slot_id               # top-2 of key << 4 | slot
            top = np.sort(v, axis=1)
            t1, t2 = top[:, -1], top[:, -2]
            k1, k2, slot = t1 >> 4, t2 >> 4, t1 & 15
            s = (k2 >> logM) + (rows <= (k2 & k_known))   # first visit of the check strictly after k2
            cand = (s << logM) | rows
            inrange = (s <= max_sweeps) & (k2 != K_INF)
            better = inrange & (cand < k1)
            target = nb[lane, slot]
            dirty[ch] = False
            if better.any():
                before = key[target[better]].copy()
                np.minimum.at(key, target[better], cand[better])    # min-wins write
                for j in np.unique(target[better][key[target[better]] < before]):
                    dirty[tab.readers[int(j)]] = True
            fire[rows] = np.where(inrange & (cand == key[target]), target, -1)
            clean = 0 if better.any() else clean + 1   # improved and not evaluated again: not clean itself
            ch = (ch + 1) % nch
    keys = key[:n]
    unknown = keys == K_INF
    solved = erased & ~unknown
    smax = int((keys[solved] >> logM).max()) if solved.any() else 0
    iterations = max(1, smax) if not unknown.any() else max_sweeps
    checks = np.flatnonzero(fire >= 0)
    checks = checks[np.argsort(key[fire[checks]], kind="stable")]
    return {"keys": keys, "pairs": [(int(c), int(fire[c])) for c in checks], "iterations": iterations,
            "residual": np.flatnonzero(unknown), "evaluations": evaluations, "capped": capped}


def apply_pairs(tab, pairs, sym, erased):
    """The solves in time order on the bytes of one frame ([n] or [n, S]): y(e) = inv(H(i,e)) * sum_{j != e} H(i,j) y(j)
    (...Decoder.m:39-47).  Symbols that stay unknown are 0."""
    y = np.array(sym, dtype=np.uint8, copy=True)
    y[np.asarray(erased).astype(bool)] = 0
    for chk, e in pairs:
        nb, cf = tab.nbr[chk], tab.coef[chk]
        acc = np.zeros(y.shape[1:], dtype=np.uint8)
        he = 0
        for j, h in zip(nb, cf):
            if j == e:
                he = int(h)
            elif j < tab.n:
                acc ^= MUL[int(h)][y[j]]
        y[e] = MUL[int(INV[he])][acc]
    return y


def batch_rounds(tab, pairs, erased):
    """The kernel takes the solves 64 at a time in time order (dependency levels in mode 2, the apply phase in mode 0); in every
    round each unfinished step of the batch reads its inputs and finishes if all of them are valid.  Returns the largest number of
    rounds a batch needs: the earliest unfinished step always is ready, so 64 at most -- the loops' `guard > 64` is never reached."""
    valid = np.append(~np.asarray(erased).astype(bool), True)
    worst = 0
    for b0 in range(0, len(pairs), CHUNK):
        todo = list(pairs[b0:b0 + CHUNK])
        rounds = 0
        while todo:
            ready = [(c, e) for c, e in todo if all(valid[j] for j in tab.nbr[c] if j != e)]   # all lanes read, then they write
            if not ready:
                return None                                                                    # not a valid time order
            for _, e in ready:
                valid[e] = True
            todo = [p for p in todo if p not in ready]
            rounds += 1
        worst = max(worst, rounds)
    return worst


# ---- code families ----------------------------------------------------------------------------------------------------------------
def _code(n, k, rows, rng):
    row_ptr, cols, coefs = [0], [], []
    for c in rows:
        cols += c
        coefs += rng.integers(1, 256, size=len(c)).tolist()
        row_ptr.append(len(cols))
    return codes.Code(n, k, np.array(row_ptr, dtype=np.uint32), np.array(cols, dtype=np.uint16), np.array(coefs, dtype=np.uint8))


def block_staircase(rng, m, k, deg, restart_every):
    """Check i = `deg` random source columns + parity i - 1 + parity i, without parity i - 1 where i is a multiple of
    `restart_every`: chains of that length, several of them in one chunk of 64 checks when it is short.  Triangle form."""
    rows = []
    for i in range(m):
        c = sorted(rng.choice(k, size=min(deg, k), replace=False).tolist())
        if i % restart_every:
            c.append(k + i - 1)
        rows.append(c + [k + i])
    return _code(k + m, k, rows, rng)


def staircase(rng, m, k, deg):
    """Dual-diagonal (IRA-style) parity part: one chain through all m checks.  With all parity erased the reference solves it in
    a single sweep; the relaxation settles one check of a chunk per pass."""
    return block_staircase(rng, m, k, deg, m + 1)


def anti_staircase(rng, m, k, deg):
    """Check i = `deg` random source columns + parity i + parity i + 1 (the last check: parity m - 1 only): the chain runs AGAINST
    the sweep order, the reference solves one parity symbol per sweep and stops at max_sweeps.  Not triangle form: no systematic
    encoder, codewords come from `codeword_by_sweeps`."""
    rows = []
    for i in range(m):
        c = sorted(rng.choice(k, size=min(deg, k), replace=False).tolist()) + [k + i]
        if i + 1 < m:
            c.append(k + i + 1)
        rows.append(c)
    return _code(k + m, k, rows, rng)


def random_triangle_code(rng, n, k, deg):
    """(n-k) x n, parity part lower triangular with a non-zero diagonal (row i ends in column k+i), random GF(256) coefficients;
    long dependency chains on purpose: every row takes its previous parity symbol with probability 0.8."""
    m = n - k
    row_ptr, cols, coefs = [0], [], []
    for r in range(m):
        c = set(rng.choice(k, size=min(deg, k), replace=False).tolist())
        if r > 0 and rng.random() < 0.8:
            c.add(k + r - 1)
        for j in rng.choice(max(r, 1), size=min(2, r), replace=False).tolist() if r > 1 else []:
            c.add(k + j)
        c = sorted(c) + [k + r]
        cols += c
        coefs += rng.integers(1, 256, size=len(c)).tolist()
        row_ptr.append(len(cols))
    return codes.Code(n, k, np.array(row_ptr, dtype=np.uint32), np.array(cols, dtype=np.uint16), np.array(coefs, dtype=np.uint8))


def is_triangle(code):
    """Row i ends in column k + i: the form the systematic encoders need."""
    rp = code.row_ptr.astype(np.int64)
    return all(rp[r + 1] > rp[r] and int(code.cols[rp[r + 1] - 1]) == code.k + r for r in range(code.m))


def codeword_by_sweeps(oc, code, source):
    """Codeword of a code whose parity part a sweep decoder can peel from the source symbols alone (every family here), made by
    the oracle's own sweeps: all parity erased, as many sweeps as there are checks.  source [k] or [k, S]."""
    source = np.asarray(source, dtype=np.uint8)
    sym = np.zeros((code.n,) + source.shape[1:], dtype=np.uint8)
    sym[:code.k] = source
    era = np.zeros(code.n, dtype=np.uint8)
    era[code.k:] = 1
    out, oe, _, _, _ = oc.decode_packets(sym.reshape(code.n, -1), era, itenum=code.m, do_ml=0)
    assert not oe.any()
    return out.reshape(sym.shape)


def syndrome(code, cw):
    """H * cw over GF(256) for one frame [n] or [n, S]."""
    cw = np.asarray(cw, dtype=np.uint8)
    rp = code.row_ptr.astype(np.int64)
    out = np.zeros((code.m,) + cw.shape[1:], dtype=np.uint8)
    for r in range(code.m):
        for e in range(int(rp[r]), int(rp[r + 1])):
            out[r] ^= MUL[int(code.coefs[e])][cw[int(code.cols[e])]]
    return out


# ---- erasure patterns -------------------------------------------------------------------------------------------------------------
PATTERNS = ("all_parity", "parity_run", "every_second_parity", "all_parity_and_sources", "all_clear", "all_erased",
            "parity_run_and_its_source", "every_second_parity_and_sources")


def structured_erasures(rng, code):
    """[len(PATTERNS), n] erasure flags, one frame per pattern:
       all_parity                        every parity symbol
       parity_run                        one run of 70..200 parity symbols (fewer checks: what fits): it crosses a border of 64 checks
       every_second_parity               parity 1, 3, 5, ...
       all_parity_and_sources            every parity symbol + two source symbols whose first check comes late: the sweeps stop at
                                         that check, a SMALL residual system with more unknowns than equations is left
       all_clear / all_erased
       parity_run_and_its_source         a run + a source symbol that is in the run's first check and in no other (where the code
                                         has one): solvable only backwards from the run's end, one symbol per sweep -- a residual
                                         of full rank when the sweeps run out
       every_second_parity_and_sources   parity 1, 3, ... + three random source symbols"""
    n, k, m = code.n, code.k, code.m
    rp = code.row_ptr.astype(np.int64)
    era = np.zeros((len(PATTERNS), n), dtype=np.uint8)

    def run_length():
        return int(min(rng.integers(70, 201), max(1, m - 2)))     # 64 checks in a row or more always cross a border

    first_check = np.full(k, m, dtype=np.int64)           # first check of every source symbol (m: in no check)
    for r in range(m - 1, -1, -1):
        c = code.cols[rp[r]:rp[r + 1]].astype(np.int64)
        first_check[c[c < k]] = r
    covered = np.flatnonzero(first_check < m)
    late = covered[np.argsort(first_check[covered], kind="stable")[-2:]]

    era[0, k:] = 1
    l0 = run_length()
    s0 = int(rng.integers(0, m - l0))
    era[1, k + s0:k + s0 + l0] = 1
    era[2, k + 1::2] = 1
    era[3, k:] = 1
    era[3, late] = 1
    era[5, :] = 1
    l1 = run_length()
    coldeg = np.bincount(code.cols.astype(np.int64), minlength=n)[:k]
    lone = [(int(first_check[j]), int(j)) for j in np.flatnonzero(coldeg == 1) if first_check[j] < m - l1]
    if lone:                                              # a source symbol that only the run's first check could solve
        s1, j1 = lone[int(rng.integers(len(lone)))]
    else:
        s1 = int(rng.integers(0, m - l1))
        c = code.cols[rp[s1]:rp[s1 + 1]].astype(np.int64)
        j1 = int(rng.choice(c[c < k])) if (c < k).any() else int(rng.integers(k))
    era[6, k + s1:k + s1 + l1] = 1
    era[6, j1] = 1
    era[7, k + 1::2] = 1
    era[7, rng.choice(k, size=min(3, k), replace=False)] = 1
    return era


def corrupt(rng, sym, era):
    """Two received symbols of every third frame changed: those frames are not codewords."""
    for f in range(1, sym.shape[0], 3):
        known = np.flatnonzero(era[f] == 0)
        if known.size >= 2:
            for j in rng.choice(known, size=2, replace=False):
                sym[f, j] ^= 0x21
    return sym


# ---- the families the tests run: name -> (seed, builder) --------------------------------------------------------------------------
def _families():
    fam = {}
    for m in (320, 896, 1000, 1024, 2048, 4096):
        fam["staircase_m%d" % m] = (m, lambda rng, m=m: staircase(rng, m, m, 4))
    fam["staircase_n_odd"] = (11, lambda rng: staircase(rng, 450, 453, 4))          # n = 903: the flag loop without 64-bit loads
    fam["staircase_m40"] = (12, lambda rng: staircase(rng, 40, 56, 4))              # fewer checks than a wavefront has lanes
    fam["block_staircase_16"] = (13, lambda rng: block_staircase(rng, 1024, 1024, 4, 16))
    fam["block_staircase_100"] = (14, lambda rng: block_staircase(rng, 1024, 1024, 4, 100))
    fam["anti_staircase_m128"] = (15, lambda rng: anti_staircase(rng, 128, 128, 4))
    fam["anti_staircase_m256"] = (16, lambda rng: anti_staircase(rng, 256, 256, 4))
    fam["random_triangle_2560"] = (17, lambda rng: random_triangle_code(rng, 2560, 1280, 9))
    return fam


FAMILIES = _families()
BUILTIN = (0, 1, 2, 3)


def family_code(name):
    seed, build = FAMILIES[name]
    return build(np.random.default_rng(7000 + seed))


def sweep_caps(m):
    """max_sweeps of the tests that the relaxation takes: 1, 3, 10 and the largest value whose keys fit."""
    return sorted({s for s in (1, 3, 10) if fits(m, s)} | {largest_fitting_sweeps(m)})


if __name__ == "__main__":
    # evaluations against the budget for the staircases: the table of DESIGN.md section 4.1b
    for name_ in [a for a in FAMILIES if a.startswith("staircase_m")]:
        code_ = family_code(name_)
        tab_ = Tables(code_)
        era_ = np.zeros(code_.n, dtype=np.uint8)
        era_[code_.k:] = 1
        for ms_ in (1, 10):
            r_ = relax(tab_, era_, ms_)
            old_ = tab_.nch * ((ms_ + 2) * 64 + 64)
            print("%-16s max_sweeps %2d  evaluations %7d  budget %7d  (round 4's cap: %6d)  iterations %d" %
                  (name_, ms_, r_["evaluations"], eval_budget(tab_.nch, code_.m, ms_), old_, r_["iterations"]))
