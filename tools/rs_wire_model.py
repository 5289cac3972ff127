"""numpy model of Reed-Solomon on the FEC wire (include/ldpc_erasure_amd_rs_wire.h), from parts that exist on their own: the oracle's
RS encoder and decoder (oracle/oracle_py.py), the interleaver's order (tools/interleave_model.py) and the windowed receiver's rule
(tools/rx_window_model.py).  A second statement of ldpc_amd_fec_rs_encode_packets_dev and ldpc_amd_fec_rxw_dev_rs_decode_many.

  send(g, source, block0, depth, fec_class=2)        source uint8 [B][k][S] -> wire packets uint8 [B n][8 + S] in depth-`depth` order
  Receiver(g, S, W, A, D)                            .push(packets, max_blocks) -> (blocks, consumed);  .flush() -> blocks
  receive(g, packets, W, A, D)                       one call and the flush: (blocks of the call, blocks of the flush, Window)
  select_first_k(erased, k)                          the first k received positions of a block, or None below k

A block is Block(number, msg uint8 [k][S], received, status): the first k received symbols go to the decoder
(ReedSolomonErasureCodes.m:78-81); a block that received fewer than k is zeros with status 1 (RS_ST_SHORT).
"""
import collections
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.dirname(_HERE))
import interleave_model as im  # noqa: E402
import rx_window_model as wm  # noqa: E402
from oracle import oracle_py  # noqa: E402

FEC_CLASS_RS = 2
ST_DECODED, ST_SHORT = 0, 1
Block = collections.namedtuple("Block", "number msg received status")


def encode(g, source):
    """source uint8 [B][k][S] -> codewords [B][n][S], byte column by byte column through the oracle."""
    source = np.asarray(source, dtype=np.uint8)
    B, k, S = source.shape
    cw = np.zeros((B, g.shape[1], S), dtype=np.uint8)
    for b in range(B):
        for s in range(S):
            cw[b, :, s] = oracle_py.rs_encode(g, np.ascontiguousarray(source[b, :, s]))
    return cw


def packetize(cw, block0, fec_class=FEC_CLASS_RS):
    """codewords [B][n][S] -> straight-order packets [B n][8 + S]: {symbol:16 | block:8 | class:8}, little endian, in both header halves."""
    B, n, S = cw.shape
    pk = np.zeros((B * n, 8 + S), dtype=np.uint8)
    blk = (block0 + np.repeat(np.arange(B), n)) & 0xFF
    sym = np.tile(np.arange(n), B)
    pk[:, 0], pk[:, 1], pk[:, 2], pk[:, 3] = sym & 0xFF, sym >> 8, blk, fec_class
    pk[:, 4:8] = pk[:, 0:4]
    pk[:, 8:] = cw.reshape(B * n, S)
    return pk


def send(g, source, block0, depth, fec_class=FEC_CLASS_RS):
    return im.interleave(packetize(encode(g, source), block0, fec_class), g.shape[1], block0, depth)


def select_first_k(erased, k):
    pos = np.flatnonzero(np.asarray(erased) == 0)
    return (pos[:k], pos.shape[0]) if pos.shape[0] >= k else (None, pos.shape[0])


def decode_planes(g, sym, erased):
    """sym [B][n][S], erased [B][n] -> (msg [B][k][S], received [B], status [B]) by the first-k rule and the oracle's decoder."""
    k = g.shape[0]
    B, _, S = sym.shape
    msg = np.zeros((B, k, S), dtype=np.uint8)
    received, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        pos, received[b] = select_first_k(erased[b], k)
        if pos is None:
            status[b] = ST_SHORT
            continue
        for s in range(S):
            m, rc = oracle_py.rs_decode(g, pos, np.ascontiguousarray(sym[b, pos, s]))
            assert rc == 0
            msg[b, :, s] = m
    return msg, received, status


class Receiver:
    def __init__(self, g, S, W, A, D=1):
        self.g, self.S = g, S
        self.k, self.n = g.shape
        self.win = wm.Window(self.n, self.k, W, A, D)
        self._packets = np.zeros((0, 8 + S), dtype=np.uint8)   # every packet seen: the model's winners are indices into it

    def _blocks(self, closed):
        numbers, sym, er = wm.planes(closed, self._packets, self.n)
        msg, received, status = decode_planes(self.g, sym, er)
        return [Block(int(numbers[j]), msg[j], int(received[j]), int(status[j])) for j in range(len(closed))]

    def push(self, packets, max_blocks=1 << 30):
        packets = np.asarray(packets, dtype=np.uint8)
        blk, sym = wm.headers(packets)
        closed, used = self.win.push_many(blk, sym, max_blocks)
        self._packets = np.concatenate([self._packets, packets[:used]])
        return self._blocks(closed), used

    def flush(self):
        return self._blocks(self.win.flush())


def receive(g, packets, W, A, D=1):
    rx = Receiver(g, packets.shape[1] - 8, W, A, D)
    blocks, used = rx.push(packets)
    assert used == packets.shape[0]
    return blocks, rx.flush(), rx.win
