"""The datagram symbol format of include/ldpc_erasure_amd_datagrams.h restated in plain numpy: the yardstick for the kernels of
csrc/datagram_dev.hip (tests/test_gpu_datagrams.py compares byte for byte) and for ldpc_amd_fec_dgram_wire_len.

A datagram symbol is a row of S bytes (S a multiple of 4, at least 8): bytes 0..3 the length L as a little-endian uint32, bytes
4..4+L-1 the datagram, every other byte zero, 0 <= L <= S - 4; L == 0 is a filler.  Datagram i is row i of source [F][k][S],
F = ceil(N / k); the last frame is completed with fillers."""
import numpy as np

PREFIX = 4
FEC_HEADER = 8
DELIVERED, FILLER, LOST, MALFORMED = 0, 1, 2, 3
CONTEXT_BYTES = 112   # the reference's context packet: 28 words (OpenCL/device/ldpc_erasure_encoder_VITA_in_UDP_out.cl:140-162)


def _check(offset, S):
    off = np.asarray(offset, dtype=np.int64)
    if off.ndim != 1 or off.shape[0] < 1:
        raise ValueError("offset must hold N + 1 >= 1 entries")
    if S < 8 or S % 4:
        raise ValueError("S must be a multiple of 4 that is at least 8")
    ln = np.diff(off)
    if off[0] < 0 or (ln < 0).any():
        raise ValueError("offsets must be non-negative and non-decreasing")
    if (ln > S - PREFIX).any():
        raise ValueError(f"datagram {int(np.argmax(ln > S - PREFIX))} is longer than S - 4")
    return off, ln


def pack(data, offset, k, S):
    """data uint8 1-D, datagram i = data[offset[i]:offset[i+1]] -> source uint8 [F][k][S]."""
    off, ln = _check(offset, S)
    data = np.asarray(data, dtype=np.uint8)
    N = ln.shape[0]
    F = -(-N // k)
    rows = np.zeros((F * k, S), dtype=np.uint8)
    rows[:N, :PREFIX] = (ln[:, None] >> (8 * np.arange(PREFIX))) & 0xFF   # little-endian
    put = np.arange(S - PREFIX)[None, :] < ln[:, None]                     # row-major: the datagrams in order, they lie back to back
    rows[:N, PREFIX:][put] = data[off[0]:off[N]]
    return rows.reshape(F, k, S)


def unpack(frames, k, erased=None):
    """frames uint8 [B][n][S], erased uint8 [B][n] or None -> (bytes uint8 [total], offset int64 [B*k+1], state uint8 [B*k]): rows
    0..k-1 of every frame in order; a row is LOST where its flag is set (its prefix is not looked at), FILLER for L == 0, MALFORMED
    for L > S - 4, else DELIVERED and its L bytes are appended."""
    frames = np.asarray(frames, dtype=np.uint8)
    B, n, S = frames.shape
    rows = frames[:, :k].reshape(B * k, S)
    L = rows[:, :PREFIX].astype(np.int64) @ (1 << (8 * np.arange(PREFIX, dtype=np.int64)))   # little-endian
    lost = np.zeros(B * k, dtype=bool) if erased is None else np.asarray(erased)[:, :k].reshape(B * k) != 0
    state = np.where(lost, LOST, np.where(L == 0, FILLER, np.where(L > S - PREFIX, MALFORMED, DELIVERED))).astype(np.uint8)
    ln = np.where(state == DELIVERED, L, 0)
    offset = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    take = np.arange(S - PREFIX)[None, :] < ln[:, None]   # row-major: the rows in order, each one's bytes in order
    return rows[:, PREFIX:][take], offset, state


def wire_len(offset, n, k, S):
    """int32 [F*n]: the bytes of packet f * n + i that have to be transmitted -- 8 + 4 + L for a source row, 8 + S for a repair row."""
    off, ln = _check(offset, S)
    if k < 1 or n < k:
        raise ValueError("need 1 <= k <= n")
    N = ln.shape[0]
    F = -(-N // k)
    w = np.full((F, n), FEC_HEADER + S, dtype=np.int32)
    src = np.full(F * k, FEC_HEADER + PREFIX, dtype=np.int32)
    src[:N] += ln.astype(np.int32)
    w[:, :k] = src.reshape(F, k)
    return w.reshape(-1)


def difi_mix(rng, N, S):
    """(data uint8 1-D, offset int64 [N+1]) of N datagrams in the reference's mix: one context datagram of 112 bytes, then 16 data
    datagrams of S - 4 bytes, and so on; random contents."""
    if S - PREFIX < CONTEXT_BYTES:
        raise ValueError("S - 4 must hold a context packet of 112 bytes")
    ln = np.full(N, S - PREFIX, dtype=np.int64)
    ln[::17] = CONTEXT_BYTES
    offset = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    return rng.integers(0, 256, size=int(offset[-1]), dtype=np.uint8), offset
