"""The ground under tests/test_gpu_address_range.py, on the host alone.

1. Tiling is sound: the oracle run DIRECTLY at S = 3 * 4080 + 256 (and at a word-form S, a multiple of 4 that is no multiple of 16)
   on a lane-tiled input returns the lane tiling of its S = 4080 result -- decode (codewords, non-codewords, status 0, 1, 2 and 3),
   encode and Reed-Solomon decode.  The GPU test may therefore compare a huge-S result tile by tile with the small one.
2. The erasure patterns chosen for the (2040,1530) code give the status classes the GPU test needs (message passing completes in
   few steps / in many steps, ML solved, rank deficient, ML skipped), so that test cannot lose a class unnoticed.
3. The edge-size functions of tools/address_range.py return sizes on the stated side of each limit."""
import numpy as np
import pytest

import address_range_cases as cases
from address_range_cases import ar

P = ar.P
S_DIRECT = 3 * P + 256     # three full tiles and a ragged one
S_WORDS = S_DIRECT + 4     # the word form


def test_no_power_of_two_is_a_multiple_of_the_period():
    assert P % 16 == 0 and (P // 16) % 2 == 1
    for e in range(4, 40):
        assert (1 << e) % P != 0
        # ... and lanes a power of two apart differ in the small problems: their content is random bytes per lane
    assert ar.PF in (2, 3, 5, 7, 11, 13)


@pytest.mark.parametrize("which,S", [("r300", S_DIRECT), ("r300", S_WORDS), ("r64", S_DIRECT), ("r3", S_DIRECT)])
def test_light_codes_direct_equals_tiled(which, S):
    c = cases.light_case(which)
    code, oc = cases.get_code(which)
    # encode
    src_big = ar.tile_lanes(c["src"], S)
    for f in range(2):
        assert ar.lanes_equal(oc.encode(src_big[f]), c["cw"][f]), f"encode, frame {f}"
    # decode: a codeword and a non-codeword
    out, sw, res, st = cases.oracle_decode(oc, ar.tile_lanes(c["sym"], S), c["era"])
    assert ar.lanes_equal(out, c["want"][0])
    for a, b in zip((sw, res, st), c["want"][1:]):
        assert np.array_equal(a, b)
    # the non-codeword really is none: the decode of frame 1 does not return the transmitted codeword
    assert not np.array_equal(c["want"][0][1], c["cw"][1]) and np.array_equal(c["want"][0][0], c["cw"][0])


def test_status_classes_of_the_2040_1530_patterns():
    code, oc = cases.get_code(cases.B_CODE)
    pat = cases.b_patterns()
    era = np.stack([pat[c] for c in cases.B_CLASSES])
    _, _, res, st = oc.decode_batch_s1(np.zeros_like(era), era)
    steps = era.sum(1) - res
    got = dict(zip(cases.B_CLASSES, zip(st.tolist(), steps.tolist())))
    print(got)
    assert got["lo"][0] == 0 and 1 <= got["lo"][1] <= cases.B_LOW
    assert got["hi"][0] == 0 and got["hi"][1] >= cases.B_HIGH
    assert got["ml1"][0] == 1 and got["ml2"][0] == 2
    _, _, _, st0 = oc.decode_batch_s1(np.zeros_like(era), era, do_ml=0)
    assert st0.tolist() == [0, 0, 3, 3]
    # every run of the GPU test: its statuses, and all of 0..3 between them
    c = cases.b_case()
    seen = set()
    for frames, do_ml in cases.B_RUNS:
        st_run = cases.b_run(c, frames, do_ml)[2][3].tolist()
        want = [{"lo": 0, "hi": 0, "ml1": 1, "nc": 1, "ml2": 2}[x] for x in frames]
        assert st_run == [w if do_ml or w == 0 else 3 for w in want], (frames, do_ml, st_run)
        seen |= set(st_run)
    assert seen == {0, 1, 2, 3}


def test_2040_1530_direct_equals_tiled():
    c = cases.b_case()
    code, oc = cases.get_code(cases.B_CODE)
    sym_big = ar.tile_lanes(c["sym"], S_DIRECT)
    for do_ml in (1, 0):
        want = c["want1" if do_ml else "want0"]
        out, sw, res, st = cases.oracle_decode(oc, sym_big, c["era"], do_ml=do_ml)
        bad = [f for f in range(out.shape[0]) if not ar.lanes_equal(out[f], want[0][f])]
        assert not bad, f"do_ml={do_ml}: frames {bad} (status {st[bad].tolist()})"
        for a, b in zip((sw, res, st), want[1:]):
            assert np.array_equal(a, b)
    nc = cases.B_FRAMES.index("nc")
    assert not np.array_equal(c["want1"][0][nc], c["cw"][nc])
    assert ar.lanes_equal(oc.encode(ar.tile_lanes(c["src"][:1], S_DIRECT)[0]), c["cw"][0])


def test_rs_direct_equals_tiled():
    from oracle import oracle_py
    c = cases.rs_case()
    g = c["g"]
    val_big = ar.tile_lanes(c["val"], S_DIRECT)
    src_big = ar.tile_lanes(c["src"], S_DIRECT)
    for b in range(2):
        msg = np.stack([oracle_py.rs_decode(g, c["idx"][b], np.ascontiguousarray(val_big[b, :, s]))[0] for s in range(S_DIRECT)], axis=1)
        assert ar.lanes_equal(msg, c["msg"][b]) and np.array_equal(c["msg"][b], c["src"][b])
        cw = np.stack([oracle_py.rs_encode(g, np.ascontiguousarray(src_big[b, :, s])) for s in range(S_DIRECT)], axis=1)
        assert ar.lanes_equal(cw, c["cw"][b])
    assert c["received"].tolist() == [cases.RS_N - 32, cases.RS_K - 3] and not c["fmsg"][1].any()


def test_frame_tiling():
    small = np.arange(ar.PF * 3, dtype=np.uint8).reshape(ar.PF, 3)
    big = ar.tile_frames(small, 2 * ar.PF + 3)
    assert all(np.array_equal(big[f], small[f % ar.PF]) for f in range(big.shape[0]))
    c = cases.batch_case(1)
    assert set(c["want"][3].tolist()) >= {0, 1}


def test_torch_tiling_equals_numpy_tiling():
    """The device-side fill and comparison functions, on CPU tensors: a ragged last tile, more than one comparison group, a
    mismatch in the first, a middle and the ragged tile, views with a row stride (the payload of a packet array)."""
    import torch
    rng = np.random.default_rng(1)
    period, S = 48, 5 * 48 + 20
    small = rng.integers(0, 256, (2, 3, period), dtype=np.uint8)
    want = torch.from_numpy(ar.tile_lanes(small, S, period))
    big = torch.zeros((2, 3, 8 + S), dtype=torch.uint8)[:, :, 8:]
    ar.fill_lanes(big, torch.from_numpy(small))
    assert torch.equal(big, want)
    old = ar._CHUNK
    ar._CHUNK = 2 * 3 * period * 2          # two tiles per group
    try:
        assert ar.lanes_mismatch(big, torch.from_numpy(small)) is None
        for s in (0, 2 * period + 5, S - 1):
            big[1, 2, s] ^= 1
            assert ar.lanes_mismatch(big, torch.from_numpy(small)) == (1, 2, s // period, s % period)
            big[1, 2, s] ^= 1
        fs = rng.integers(0, 256, (ar.PF, 5), dtype=np.uint8)
        F = 3 * ar.PF + 4
        fb = ar.fill_frames(torch.zeros((F, 5), dtype=torch.uint8), torch.from_numpy(fs))
        assert torch.equal(fb, torch.from_numpy(ar.tile_frames(fs, F)))
        ar._CHUNK = ar.PF * 5 * 2
        assert ar.frames_mismatch(fb, torch.from_numpy(fs)) is None
        w = torch.from_numpy(ar.tile_frames(fs[:, 0].copy(), F))
        assert ar.frames_mismatch(w, torch.from_numpy(fs[:, 0].copy())) is None
        for f in (0, ar.PF + 2, F - 1):
            fb[f, 4] ^= 1
            assert ar.frames_mismatch(fb, torch.from_numpy(fs)) == f
            fb[f, 4] ^= 1
            w[f] ^= 1
            assert ar.frames_mismatch(w, torch.from_numpy(fs[:, 0].copy())) == f
            w[f] ^= 1
    finally:
        ar._CHUNK = old


def test_edge_sizes_are_on_the_stated_side():
    for n in (300, 64, 2040, 255):
        for lim in (ar.LIM_SIGN, ar.LIM_OFFSET):
            for extra in (0, 8):
                lo, hi = ar.edge_pair(lim, n, extra)
                assert lo % 256 == 0 and hi == lo + 256
                assert n * (extra + lo) < lim <= n * (extra + hi)
                assert n * (extra + lo + 255) >= lim - 256 * n          # the LAST multiple below
    assert ar.edge_pair(ar.LIM_MUL24) == ((1 << 24) - 256, 1 << 24)
    assert ar.edge_pair(ar.LIM_MUL24, extra=8) == ((1 << 24) - 256, 1 << 24)
    assert ar.edge_pair(ar.LIM_RS_ROW) == ((1 << 23) - 256, 1 << 23)
    # where each code's two limits lie: (300,200) meets n * S first, (64,44) meets S < 2^24 first
    assert ar.first_from(ar.LIM_OFFSET, 300) < ar.LIM_MUL24 and 64 * ar.LIM_MUL24 < ar.LIM_OFFSET
    w = ar.word_size_above(ar.LIM_SIGN, 300)
    assert w % 4 == 0 and w % 16 != 0 and 300 * w >= ar.LIM_SIGN and 300 * w < ar.LIM_OFFSET
    for S in (1024, ar.last_below(ar.LIM_OFFSET, 300, 8)):
        lo, hi = ar.stride_pair(S)
        assert lo * (8 + S) < ar.LIM_OFFSET <= hi * (8 + S)
    for fb in (2040, 2040 * 1024, 300 * 1024):
        F = ar.frames_from(ar.LIM_OFFSET, fb)
        assert (F - 1) * fb >= ar.LIM_OFFSET > (F - 2) * fb
