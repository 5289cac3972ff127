"""Shapes and inputs shared by tests/test_link_cpu.py, tests/test_link_abi.py and tests/test_gpu_link.py (numpy and the package's
host side only): the plan grid of the link emulator (include/ldpc_erasure_amd_link.h) and the variants run at every point of it."""
import os
import sys

import numpy as np

from ldpc_erasure_codes_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import link_model as lm  # noqa: E402

TILE = 256                                     # kTile of link_dev.hip
PS = [0, 1, 255, 256, 257, 513, 3000]          # below, at and above one tile, more than one workgroup, no multiple of the tile
WS = [0, 1, 63, 64, 255, 256, 257, 4096]       # W + 1 below, at and above a wave and a tile; 4096 with P = 257: a halo wider than the call
FIRSTS = [0, (1 << 32) - 3, 1 << 40]           # 2g + c crosses 2^33 inside the call; beyond 32 bits altogether
DUPS = [0.0, 0.02, 1.0]
LOSTS = ["none", "all", "uniform", "bursty"]
GE = (0.13, 0.8, 10.0)                         # alpha, beta, good_transition_bias of the Gilbert-Elliott stream
LOSS_SEED = 77

# (lost kind, dup, first, bad_sym, foreign, flags): every lost kind with every dup, the firsts and both damage kinds spread over them.
# The Gilbert-Elliott generators (numpy and device) run their chain from global symbol 0, so that loss is drawn at first = 0 only.
VARIANTS = [(lost, dup, 0 if lost == "bursty" else FIRSTS[(a + b) % 3], (0.5, 0.0, 0.005)[(a + b) % 3], (0.5, 0.0, 0.005)[(a + b) % 3], (a + b) & 1)
            for a, lost in enumerate(LOSTS) for b, dup in enumerate(DUPS)]
GRID = [(P, W) for P in PS for W in WS]


def lost_host(kind, P, first):
    """The loss input of a variant, on the host (None: nothing is lost)."""
    if kind == "none":
        return None
    if kind == "all":
        return np.ones(P, dtype=np.uint8)
    if kind == "uniform":
        return synth.erasures_uniform(LOSS_SEED, first, P, 1, 0.10).reshape(P)
    assert kind == "bursty" and first == 0
    return synth.erasures_bursty(LOSS_SEED, 0, P, 1, *GE).reshape(P)


def params_of(variant, W, seed):
    _, dup, first, bad, foreign, flags = variant
    return lm.Params(seed=seed, first=first, window=W, flags=flags, dup=dup, bad_sym=bad, foreign=foreign)


def cpu_variant(P, W):
    """One variant per grid point for the CPU tests, all of them used over the grid."""
    return VARIANTS[(PS.index(P) * len(WS) + WS.index(W)) % len(VARIANTS)]


def random_packets(rng, P, S):
    """P packets of noise with plausible headers (symbol < 2040, both halves equal)."""
    pk = rng.integers(0, 256, size=(P, 8 + S), dtype=np.uint8)
    pk[:, 4:8] = pk[:, 0:4]
    return pk


# ---- the end-to-end runs: link parameters and loss seeds for which the host reference alone (api.FecRx fed the model's arriving
# packets, the oracle on the closed blocks' patterns) closes and decodes every block but the last open one.  5 % of 2040 leaves about
# 1938 packets a block, above the close rule's k + 0.2 (n - k) = 1632.  tests/test_link_cpu.py checks it.
E2E_LINK = dict(window=120, dup=0.02, bad_sym=0.005, foreign=0.005, dup_flip=True)
E2E_FIXED = dict(code=1, S=16, F=6, seed=1, loss_seed=101, loss=0.05)                 # the built-in (2040, 1530) code
E2E_FLOWS = dict(S=16, nflows=3, per=4, seed=1, loss_seed=101, loss=0.05, window=30, block0=(0, 50, 100))   # code_helpers.random_code()


def e2e_params(seed, window=None, dup_flip=None):
    flip = E2E_LINK["dup_flip"] if dup_flip is None else dup_flip
    return lm.Params(seed=seed, first=0, window=E2E_LINK["window"] if window is None else window, flags=lm.DUP_FLIP if flip else 0,
                     dup=E2E_LINK["dup"], bad_sym=E2E_LINK["bad_sym"], foreign=E2E_LINK["foreign"])


def e2e_model(packets, pr, loss_seed, loss, flow_of=None):
    """The model's arriving packets (and their flows) for host packets in send order: (packets_out, flow_of_out, src, fate, lost)."""
    P = packets.shape[0]
    lost = synth.erasures_uniform(loss_seed, pr.first, P, 1, loss).reshape(P)
    src, fate = lm.plan(pr, P, lost)
    out, fo = lm.apply(packets, src, fate, flow_of)
    return out, fo, src, fate, lost


def host_receiver(packets, n, k, S, max_blocks):
    """api.FecRx over the whole stream, then the flushes: (blocks [B], sym [B][n][S], erased [B][n], dropped, flushed blocks)."""
    from ldpc_erasure_codes_amd import api
    rx = api.FecRx(n, k, S)
    b, sym, er, used = rx.push_many(packets, max_blocks)
    assert used == packets.shape[0]
    blocks, syms, ers, flushed = b.tolist(), [sym], [er], 0
    while True:
        r = rx.flush()
        if r is None:
            break
        blocks.append(r[0])
        syms.append(r[1][None])
        ers.append(r[2][None])
        flushed += 1
    dropped = rx.dropped
    rx.close()
    return np.array(blocks, dtype=np.int32), np.concatenate(syms), np.concatenate(ers), dropped, flushed
