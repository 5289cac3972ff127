"""Codes built for tests, shared by CPU and GPU test modules (numpy and the package's host side only)."""
import numpy as np

from ldpc_erasure_codes_amd import codes


def random_code(n=300, k=200, coldeg=3, seed=3):
    """A random triangular (300,200) code: every source column sits in coldeg random checks, check i ends at its own parity column
    k + i and also holds the parity columns k + i - 1 and (from i = 2 on) one earlier one.  Column degrees stay far below 16, the
    scatter kernels' limit."""
    rng = np.random.default_rng(seed)
    m = n - k
    H = np.zeros((m, n), dtype=np.uint8)
    for c in range(k):
        H[rng.choice(m, size=coldeg, replace=False), c] = rng.integers(1, 256, size=coldeg)
    for i in range(m):
        H[i, k + i] = rng.integers(1, 256)
        if i >= 1:
            H[i, k + i - 1] = rng.integers(1, 256)
        if i >= 2:
            H[i, k + rng.integers(0, i - 1)] = rng.integers(1, 256)
    return codes.from_dense(H, k)
