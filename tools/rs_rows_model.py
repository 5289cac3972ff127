"""numpy model of the Reed-Solomon decoder on rows in place (include/ldpc_erasure_amd_rs_rows.h): a second statement of the plan kernel
of csrc/rs_wire_dev.hip -- vetting, selection, the per-block coefficient table -- and of its application by the stream kernel.  The
field is built here from its polynomial, the generator is the caller's (Context.rs_generator or the oracle's): nothing below calls
the oracle's decoder, so the tests can compare the two.

  vet(src, npackets, nstage_rows)          usable [B][n] bool: the word is not ERASED and names a row inside its array
  select(usable, k)                        (positions of the first k usable symbols or None, usable count) of one block
  table(g, pos)                            Plan(nsys, r, upos, D): msg[upos[u]] = sum_t D[t][u] * row_t over the k selected rows
  fetch(word, packets, stage)              the row a vetted word names
  frames(src, packets, stage)              (sym [B][n][S], erased [B][n]): the frames the words describe, erased rows zero
  decode_rows(g, src, packets, stage)      (msg [B][k][S], received [B], status [B], erased [B][n])
  bucket(r)                                the accumulator count a block of r missing source rows runs with (0: a copy)
"""
import collections

import numpy as np

PRIM_POLY = 0x171
ROW_STAGED, ROW_ERASED = 0x80000000, 0xFFFFFFFF
ST_DECODED, ST_SHORT = 0, 1
BUCKETS = (8, 16, 24, 32, 48, 64)
R_MAX = BUCKETS[-1]
Plan = collections.namedtuple("Plan", "nsys r upos D")


def _field():
    ex = np.zeros(512, dtype=np.int64)
    lg = np.zeros(256, dtype=np.int64)
    x = 1
    for i in range(255):
        ex[i] = ex[i + 255] = x
        lg[x] = i
        x <<= 1
        if x & 0x100:
            x ^= PRIM_POLY
    a = np.arange(256)
    mul = ex[lg[a][:, None] + lg[a][None, :]]
    mul[0, :] = 0
    mul[:, 0] = 0
    inv = np.zeros(256, dtype=np.uint8)
    inv[1:] = ex[(255 - lg[1:]) % 255]
    return mul.astype(np.uint8), inv


MUL, INV = _field()


def bucket(r):
    return 0 if r == 0 else next(b for b in BUCKETS if r <= b)


def vet(src, npackets, nstage_rows):
    src = np.asarray(src).astype(np.int64) & 0xFFFFFFFF
    staged = (src & ROW_STAGED) != 0
    idx = src & 0x7FFFFFFF
    return (src != ROW_ERASED) & np.where(staged, idx < nstage_rows, idx < npackets)


def select(usable, k):
    pos = np.flatnonzero(usable)
    return (pos[:k] if pos.shape[0] >= k else None), int(pos.shape[0])


def invert(M):
    """Gauss-Jordan over GF(256), the first non-zero pivot of a column; M square uint8."""
    r = M.shape[0]
    A = np.concatenate([M.astype(np.uint8), np.eye(r, dtype=np.uint8)], axis=1)
    for c in range(r):
        p = c + int(np.flatnonzero(A[c:, c])[0])   # (IndexError: singular -- not an MDS generator)
        if p != c:
            A[[c, p]] = A[[p, c]]
        A[c] = MUL[INV[A[c, c]], A[c]]
        f = A[:, c].copy()
        f[c] = 0
        A ^= MUL[f[:, None], A[c][None, :]]
    return A[:, r:]


def table(g, pos):
    """g [k][n] systematic generator, pos the k selected positions (ascending)."""
    k = g.shape[0]
    pos = np.asarray(pos)
    nsys = int((pos < k).sum())
    r = k - nsys
    upos = np.setdiff1d(np.arange(k), pos[:nsys])
    D = np.zeros((k, r), dtype=np.uint8)
    if r:
        cols = pos[nsys:]                          # codeword positions of the selected repair rows: column j_q = cols[q] - k of P
        minv = invert(g[np.ix_(upos, cols)].T)     # M[q][t] = P[u_t][j_q]
        D[nsys:] = minv.T                          # D[nsys + q][u] = Minv[u][q]
        for t in range(nsys):                      # D[t][u] = sum_q Minv[u][q] P[pos_t][j_q]
            D[t] = np.bitwise_xor.reduce(MUL[minv, g[pos[t], cols][None, :]], axis=1)
    return Plan(nsys, r, upos, D)


def fetch(word, packets, stage):
    word = int(word) & 0xFFFFFFFF
    return stage[word & 0x7FFFFFFF] if word & ROW_STAGED else packets[word, 8:]


def _arrays(packets, stage):
    S = packets.shape[1] - 8 if packets is not None else stage.shape[1]
    packets = np.zeros((0, 8 + S), np.uint8) if packets is None else np.asarray(packets)
    stage = np.zeros((0, S), np.uint8) if stage is None else np.asarray(stage)
    return S, packets, stage


def frames(src, packets, stage):
    S, packets, stage = _arrays(packets, stage)
    src = np.asarray(src)
    ok = vet(src, packets.shape[0], stage.shape[0])
    sym = np.zeros(src.shape + (S,), dtype=np.uint8)
    for b, j in zip(*np.nonzero(ok)):
        sym[b, j] = fetch(src[b, j], packets, stage)
    return sym, (~ok).astype(np.uint8)


def decode_rows(g, src, packets, stage):
    S, packets, stage = _arrays(packets, stage)
    src = np.asarray(src)
    k = g.shape[0]
    B = src.shape[0]
    ok = vet(src, packets.shape[0], stage.shape[0])
    msg = np.zeros((B, k, S), dtype=np.uint8)
    received, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        pos, received[b] = select(ok[b], k)
        if pos is None:
            status[b] = ST_SHORT
            continue
        plan = table(g, pos)
        rows = np.stack([fetch(src[b, j], packets, stage) for j in pos])   # every selected row read once, where it lies
        msg[b, pos[:plan.nsys]] = rows[:plan.nsys]
        for u in range(plan.r):
            msg[b, plan.upos[u]] = np.bitwise_xor.reduce(MUL[plan.D[:, u][:, None], rows], axis=0)
    return msg, received, status, (~ok).astype(np.uint8)
