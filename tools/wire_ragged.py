"""The trimmed wire of include/ldpc_erasure_amd_wire_ragged.h restated in plain numpy: the yardstick for the kernels of
csrc/wire_ragged_dev.hip (tests/test_gpu_wire_ragged.py compares byte for byte).

A packet is 8 + S bytes: the FEC header (bytes 0..1 the symbol number, little-endian), then the symbol.  trim cuts a source row
(symbol number below k) whose first four payload bytes read as a length L <= S - 4 to its 8 + 4 + L bytes and sends every other
packet whole; land puts datagram p = data[offset[p]:offset[p+1]] into slot p with zeros behind it, or -- where its boundaries or
its length are bad -- makes slot p eight bytes 0xFF and zeros, a header every receiver drops."""
import numpy as np

FEC_HEADER = 8
PREFIX = 4
LANDED, REJECTED = 0, 1


def _check_S(S):
    if S < 8 or S % 4:
        raise ValueError("S must be a multiple of 4 that is at least 8")


def wire_len(packets, k):
    """int64 [P]: the bytes of every packet [P][8+S] that trim sends, from the packet alone."""
    packets = np.asarray(packets, dtype=np.uint8)
    P, plen = packets.shape
    S = plen - FEC_HEADER
    _check_S(S)
    sym = packets[:, 0].astype(np.int64) | packets[:, 1].astype(np.int64) << 8
    L = packets[:, FEC_HEADER:FEC_HEADER + PREFIX].astype(np.int64) @ (1 << (8 * np.arange(PREFIX, dtype=np.int64)))   # little-endian
    return np.where((sym < k) & (L <= S - PREFIX), FEC_HEADER + PREFIX + L, plen).astype(np.int64)


def trim(packets, k):
    """packets uint8 [P][8+S] -> (bytes uint8 [total], offset int64 [P+1]): the first wire_len bytes of every packet back to back."""
    packets = np.asarray(packets, dtype=np.uint8)
    ln = wire_len(packets, k)
    offset = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    take = np.arange(packets.shape[1])[None, :] < ln[:, None]   # row-major: the packets in order, each one's bytes in order
    return packets[take], offset


def land(data, offset, nbytes, S):
    """data uint8 1-D (its first nbytes bytes count), offset int64 [P+1] -> (packets uint8 [P][8+S], state uint8 [P]).  Datagram p is
    LANDED iff 0 <= offset[p] <= offset[p+1] <= nbytes and 8 <= its length <= 8 + S; nothing of a REJECTED one is read."""
    _check_S(S)
    off = np.asarray(offset, dtype=np.int64)
    if off.ndim != 1 or off.shape[0] < 1:
        raise ValueError("offset must hold P + 1 >= 1 entries")
    data = np.asarray(data, dtype=np.uint8)
    P, plen = off.shape[0] - 1, FEC_HEADER + S
    o0, o1 = off[:-1], off[1:]
    ok = (o0 >= 0) & (o1 >= o0) & (o1 <= nbytes)
    ln = np.where(ok, o1 - np.where(ok, o0, o1), 0)     # (no difference of two wild offsets: it could overflow)
    ok &= (ln >= FEC_HEADER) & (ln <= plen)
    packets = np.zeros((P, plen), dtype=np.uint8)
    packets[~ok, :FEC_HEADER] = 0xFF
    take = np.arange(plen)[None, :] < np.where(ok, ln, 0)[:, None]
    packets[take] = data[(np.where(ok, o0, 0)[:, None] + np.arange(plen)[None, :])[take]]
    return packets, np.where(ok, LANDED, REJECTED).astype(np.uint8)
