"""CPU tests of the model of the Reed-Solomon decoder on rows in place (tools/rs_rows_model.py) over the blocks of tests/rs_rows_cases.py,
which the GPU test shares: the model's output equals the oracle's decoder behind the first-k rule (rs_wire_model.decode_planes) on
the frames the words describe, and the case list really holds every kind of block it is meant to hold."""
import numpy as np
import pytest

import rs_rows_cases as rc
import rs_wire_cases as rw

rr = rc.rr
S = 16


@pytest.fixture(scope="module", params=rc.CODES, ids=lambda c: "rs%d_%d" % c)
def blocks(request):
    n, k = request.param
    cs = rc.cases(n, k)
    built = rc.build(cs, n, k, S, seed=n + k)
    return n, k, cs, built, rc.reference(rw.generator(n, k), built)


def test_the_case_list_holds_every_kind_of_block(blocks):
    n, k, cs, built, _ = blocks
    got = rc.facts(cs, built, n, k)
    assert got >= rc.want(n, k), sorted(rc.want(n, k) - got)
    if n - k >= 49:
        assert {"bucket %d" % b for b in rr.BUCKETS} | {"bucket 0"} <= got, "RS(255,192) runs every body of the stream kernel"


def test_model_equals_the_oracle_on_the_frames_the_words_describe(blocks):
    n, k, cs, built, (msg, received, status, er) = blocks
    got = rr.decode_rows(rw.generator(n, k), built.src, built.packets, built.stage)
    for name, a, b in zip(("msg", "received", "status", "erased"), got, (msg, received, status, er)):
        assert np.array_equal(a, b), name
    short = status == rr.ST_SHORT
    assert short.any() and not msg[short].any() and (received[short] < k).all() and (received[~short] >= k).all()


def test_rows_behind_the_first_k_do_not_matter(blocks):
    n, k, cs, built, (msg, received, status, er) = blocks
    other = rc.build(cs, n, k, S, seed=n + k, garbage=99)
    assert np.array_equal(other.src, built.src)
    assert not np.array_equal(other.packets, built.packets) and not np.array_equal(other.stage, built.stage), "some rows changed"
    got = rr.decode_rows(rw.generator(n, k), other.src, other.packets, other.stage)
    assert np.array_equal(got[0], msg) and np.array_equal(got[1], received) and np.array_equal(got[2], status)


def test_vetting_takes_a_word_past_either_array_as_erased():
    src = np.array([[0, 4, 5, rr.ROW_STAGED | 2, rr.ROW_STAGED | 3, rr.ROW_ERASED, rr.ROW_STAGED | 0x7FFFFFFF]], dtype=np.uint32)
    assert rr.vet(src, 5, 3).tolist() == [[True, True, False, True, False, False, False]]
    assert not rr.vet(src, 0, 0).any()


def test_table_is_the_inverse_applied_to_a_codeword():
    """On a real codeword the table gives the source back, and its rows are what the header says: D[nsys + q][u] = Minv[u][q]."""
    n, k = 15, 11
    g = rw.generator(n, k)
    source = rw.source(1, k, 4, seed=3)
    cw = rw.rm.encode(g, source)[0]
    pos = np.array([0, 2, 3, 4, 6, 7, 8, 10, 11, 13, 14])   # source rows 1, 5, 9 missing: repair columns 0, 2, 3 stand in
    plan = rr.table(g, pos)
    assert (plan.nsys, plan.r, plan.upos.tolist()) == (8, 3, [1, 5, 9]) and plan.D.shape == (k, 3)
    M = g[np.ix_(plan.upos, pos[plan.nsys:])].T
    assert np.array_equal(plan.D[plan.nsys:].T, rr.invert(M))
    ident = np.bitwise_xor.reduce(rr.MUL[rr.invert(M)[:, :, None], M[None, :, :]], axis=1)
    assert np.array_equal(ident, np.eye(3, dtype=np.uint8))
    for u in range(3):
        assert np.array_equal(np.bitwise_xor.reduce(rr.MUL[plan.D[:, u][:, None], cw[pos]], axis=0), source[0, plan.upos[u]])


def test_buckets():
    assert [rr.bucket(r) for r in (0, 1, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 64)] == [0, 8, 8, 16, 16, 24, 24, 32, 32, 48, 48, 64, 64]
