#!/usr/bin/env python3
"""Erasure patterns with a CHOSEN number of solved steps, and an independent reference for the simplest of them.

The packet kernels (csrc/kernels.hip: ldpc_scatter_kernel, ldpc_scatter_big_kernel and their packets-in forms) switch behaviour on a
frame's number of solved steps at hard thresholds.  A channel deals step counts at random; these patterns
place a frame ON a threshold:

  parity_subset(code, t, seed, where)   exactly t PARITY symbols erased.  The built-in codes are in triangle form (check i ends at its
                                        own parity column k + i, its other parity columns lie before it), so one in-order sweep
                                        solves exactly those t symbols: t steps, sweeps = 1, residual = 0.
  exact_subset(code, E, seed)           exactly E of the n symbols erased, drawn uniformly.  Up to 0.18 n these peel completely on
                                        the built-in codes (E steps in a few sweeps); from about 0.22 n on they leave a residual
                                        system for the ML stage behind E - residual steps.
  single_sweep_reference(code, sym, erased)
                                        the bytes after ONE in-order sweep over a parity-only pattern, in numpy, with GF(256) tables
                                        built here from the polynomial 0x171 (tools/pi_model.py) -- not the library's, not the
                                        oracle's.  It is the expected output where "equals the codeword" does not apply: received
                                        symbols that are no codeword.

Test infrastructure (tests/test_step_patterns_cpu.py pins it on the oracle, tests/test_gpu_plan_edges.py uses it); numpy only, and
of the package under test it reads nothing but a codes.Code."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pi_model import INV, MUL  # noqa: E402

WHERE = ("random", "first", "last")
_MUL_FLAT = np.ascontiguousarray(MUL).reshape(-1)


def parity_subset(code, t, seed, where="random"):
    """uint8 [n] flags with exactly t of the m parity symbols erased: t random ones, the first t (every step depends on the one
    before it through the triangle: the longest chain) or the last t."""
    m = code.n - code.k
    if not 0 <= t <= m:
        raise ValueError(f"t = {t} outside 0..{m}")
    if where not in WHERE:
        raise ValueError(f"where = {where!r}, not one of {WHERE}")
    flags = np.zeros(code.n, dtype=np.uint8)
    if where == "first":
        pos = np.arange(t)
    elif where == "last":
        pos = np.arange(m - t, m)
    else:
        pos = np.random.default_rng([int(seed), int(t), 1]).choice(m, size=t, replace=False)
    flags[code.k + pos] = 1
    return flags


def exact_subset(code, E, seed):
    """uint8 [n] flags with exactly E of the n symbols erased, every E-subset equally likely."""
    if not 0 <= E <= code.n:
        raise ValueError(f"E = {E} outside 0..{code.n}")
    flags = np.zeros(code.n, dtype=np.uint8)
    flags[np.random.default_rng([int(seed), int(E), 2]).choice(code.n, size=E, replace=False)] = 1
    return flags


def is_triangle(code):
    """Check i holds its own parity column k + i and no parity column behind it."""
    rp, cols, k = code.row_ptr, code.cols, code.k
    for i in range(code.n - code.k):
        c = cols[int(rp[i]):int(rp[i + 1])]
        if (c == k + i).sum() != 1 or c.max() != k + i:
            return False
    return True


def single_sweep_reference(code, sym, erased):
    """sym uint8 [F, n, S], erased uint8 [F, n] with parity symbols only -> uint8 [F, n, S] after one in-order sweep:
    for i = 0 .. m-1, in the frames whose symbol k + i is erased, sym[k+i] = inv(h_ii) * XOR_j h_ij * sym[j] over the current values
    of the row's other symbols (the erased ones among them were solved by an earlier row: triangle form).  What an erased symbol held
    on the way in is never read."""
    sym = np.asarray(sym, dtype=np.uint8)
    erased = np.asarray(erased, dtype=np.uint8)
    F, n, S = sym.shape
    k, m = code.k, code.n - code.k
    if n != code.n or erased.shape != (F, n):
        raise ValueError("shapes do not match the code")
    if erased[:, :k].any():
        raise ValueError("single_sweep_reference: parity-only patterns")
    if not is_triangle(code):
        raise ValueError("single_sweep_reference: the code is not in triangle form")
    out = sym.copy()
    rp, cols, coefs = code.row_ptr, code.cols.astype(np.int64), code.coefs.astype(np.int64)
    for i in range(m):                                    # the only Python loop: frames and byte lanes are array axes
        fr = np.flatnonzero(erased[:, k + i])
        if fr.size == 0:
            continue
        s, e = int(rp[i]), int(rp[i + 1])
        c, h = cols[s:e], coefs[s:e]
        own = c == k + i
        oc, oh = c[~own], h[~own]
        vals = out[fr[:, None], oc[None, :], :]           # [frames, deg - 1, S]
        prod = _MUL_FLAT[(oh[None, :, None] << 8) | vals]
        acc = np.bitwise_xor.reduce(prod, axis=1)
        out[fr, k + i, :] = _MUL_FLAT[(int(INV[h[own][0]]) << 8) | acc.astype(np.int64)]
    return out


def triangle_code(n=130, k=66, rowdeg=20, seed=7):
    """A small hand-made code in triangle form: check i holds its own parity column k + i, the one before it (a chain through
    all checks) and, up to `rowdeg` entries in all, random source columns and earlier parity columns.  Returns a codes.Code."""
    from ldpc_erasure_codes_amd import codes
    rng = np.random.default_rng(seed)
    m = n - k
    H = np.zeros((m, n), dtype=np.uint8)
    for i in range(m):
        H[i, k + i] = rng.integers(1, 256)
        if i >= 1:
            H[i, k + i - 1] = rng.integers(1, 256)
        pool = np.concatenate([np.arange(k), k + np.arange(max(0, i - 1))])
        pick = rng.choice(pool, size=rowdeg - int((H[i] != 0).sum()), replace=False)
        H[i, pick] = rng.integers(1, 256, size=pick.size)
    return codes.from_dense(H, k)
