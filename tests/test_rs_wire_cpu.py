"""CPU tests of Reed-Solomon on the FEC wire (include/ldpc_erasure_amd_rs_wire.h): the numpy model of tools/rs_wire_model.py returns
what was sent, and the C host receiver followed by the oracle's decoder agrees with it block for block on a thinned stream."""
import numpy as np
import pytest

import rs_wire_cases as rw
from ldpc_erasure_codes_amd import api

rm, wm = rw.rm, rw.wm


@pytest.mark.parametrize("W,D,B", [(2, 1, 12), (32, 8, 23), (32, 16, 20)])
def test_model_returns_every_source_block_on_a_loss_free_wire(W, D, B):
    """Block 250 is off every group boundary but depth 1's: the window anchors at the group start, 248 or 240, and the slots below 250
    never fill.  Nothing can close before them, so the stream has to fit the window (B blocks do) and leaves through the flush, the
    empty leading slots as all-erased blocks.  A stream that starts on a group boundary closes block by block, as depth 1 does here."""
    n, k, S = 40, 30, 16
    g = rw.generator(n, k)
    src = rw.source(B, k, S, seed=D)
    pk = rm.send(g, src, rw.BLOCK0, D)
    assert pk.shape == (B * n, 8 + S) and set(pk[:, 3]) == {rm.FEC_CLASS_RS} and np.array_equal(pk[:, :4], pk[:, 4:8])
    numbers = (rw.BLOCK0 + np.arange(B)) & 0xFF
    assert numbers.min() == 0 and numbers.max() == 255, "the stream crosses the 8-bit wrap"
    closed, flushed, win = rm.receive(g, pk, W, 10, D)
    assert win.totals["late"] == win.totals["ahead_total"] == 0 and (len(closed) == B) == (D == 1)
    got = {b.number: b for b in closed + flushed}
    for j in range(B):
        b = got[int(numbers[j])]
        assert b.status == rm.ST_DECODED and b.received == n and np.array_equal(b.msg, src[j]), j
    lead = [b for b in closed + flushed if b.number not in set(numbers.tolist())]
    assert len(lead) == rw.BLOCK0 % D and all(b.status == rm.ST_SHORT and b.received == 0 and not b.msg.any() for b in lead)


def test_model_encoder_is_systematic_and_first_k_selection_is_the_references():
    n, k = 12, 5
    g = rw.generator(n, k)
    src = rw.source(2, k, 4, seed=1)
    cw = rm.encode(g, src)
    assert np.array_equal(cw[:, :k], src)
    er = np.zeros(n, dtype=np.uint8)
    er[[0, 2, 3]] = 1
    pos, cnt = rm.select_first_k(er, k)
    assert pos.tolist() == [1, 4, 5, 6, 7] and cnt == 9
    er[4:] = 1
    assert rm.select_first_k(er, k) == (None, 1)
    msg, received, status = rm.decode_planes(g, cw, np.stack([np.zeros(n, np.uint8), er]))
    assert np.array_equal(msg[0], src[0]) and status.tolist() == [0, 1] and received.tolist() == [n, 1] and not msg[1].any()


@pytest.mark.parametrize("W,A,D", rw.WAD)
def test_host_receiver_and_oracle_decoder_equal_the_model_on_a_thinned_stream(W, A, D):
    n, k, S = 140, 100, 16   # (a thinned block closes by the rule's second clause, which wants more than 100 later packets)
    g = rw.generator(n, k)
    B1, B2 = rw.nblocks_for(D)
    src = rw.source(B1 + B2, k, S, seed=10 + D)
    parts = rw.pieces(lambda f, cnt, b0: rm.send(g, src[f:f + cnt], b0, D), n, k, D, seed=20 + D)
    rx = rm.Receiver(g, S, W, A, D)
    handed = []
    with api.FecRxWindowHost(n, k, S, W, A, depth=D) as host:
        for pk in parts:
            closed, used = rx.push(pk)
            flushed = rx.flush()
            bl, sy, er, hused = host.push_many(pk, 1 << 20)
            fb, fs, fe = host.flush()
            assert used == hused == pk.shape[0] and host.stats() == rx.win.totals and host.state() == rx.win.state()
            for blocks, sym, era, want in ((bl, sy, er, closed), (fb, fs, fe, flushed)):
                msg, received, status = rm.decode_planes(g, sym, era)
                assert blocks.tolist() == [b.number for b in want]
                for j, b in enumerate(want):
                    assert (received[j], status[j]) == (b.received, b.status) and np.array_equal(msg[j], b.msg), (b.number, j)
            handed += closed + flushed
    decoded = [b for b in handed if b.status == rm.ST_DECODED]
    assert len(decoded) >= (B1 + B2) // 2 and any(b.status == rm.ST_SHORT for b in handed)
    model = [x for piece in rw.model_blocks(parts, n, k, W, A, D) for half in piece for x in half]
    assert rw.facts(model, n, k) == rw.WANT
    assert sorted(b.received for b in handed) == sorted(len(w_) for _, w_ in model)
