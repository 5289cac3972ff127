"""GPU tests of the multi-flow sender (include/ldpc_erasure_amd_sender_flows.h): the frames of many FEC streams encoded by one call
into one packet array, flow after flow (SEGMENTED) or one packet of every flow in turn (ROUND_ROBIN).

The expected bytes are the per-flow outputs of the single-flow call (fec_encode_packets_device, which test_gpu_sender.py pins to
the CPU oracle), placed by this file's own statement of the order: all packets sorted by (round, flow), where a flow's q-th packet
belongs to round q.  One case per path is also compared with packets built from the oracle's codewords directly.  On top of that:
which path ran, guard bands at three alignments, the first packet array beyond 2^32 bytes, two calls enqueued back to back, the
round trip through a lossy wire into FecRxFlows.decode_mixed, the block counters of FecTxFlows, and the refusals."""
import numpy as np
import pytest

from ldpc_erasure_codes_amd import api, codes
from test_gpu_sender import heavy_code, make_source, non_triangular_code, oracle_packets

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL, ENOCODE, EUNSUP = -1, -4, -5
SEG, RR = api.TX_SEGMENTED, api.TX_ROUND_ROBIN
MIB = 1 << 20


# ------------------------------------------------------------------------------------------ the order, stated independently
def wire_order(counts, n, order):
    """(perm int64 [P], flow int32 [P]): the packet at wire position p is packet perm[p] of the SEGMENTED array and belongs to
    flow[p].  ROUND_ROBIN: flow f's q-th packet (row q % n of its frame q // n) goes out in round q, flows ascending inside a
    round -- a sort of all packets by (q, f)."""
    counts = np.asarray(counts, dtype=np.int64)
    flow = np.repeat(np.arange(len(counts)), counts * n)
    if order == SEG:
        return np.arange(flow.size, dtype=np.int64), flow.astype(np.int32)
    q = np.concatenate([np.arange(c * n) for c in counts]) if flow.size else np.zeros(0, dtype=np.int64)
    perm = np.lexsort((flow, q)).astype(np.int64)
    return perm, flow[perm].astype(np.int32)


def begin_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def src_arg(src):
    return src[:, :, 0].contiguous() if src.shape[2] == 1 else src


def per_flow_packets(ctx, h, n, src, counts, classes, blocks):
    """The SEGMENTED array from one single-flow call per flow."""
    S = src.shape[2]
    fb = begin_of(counts)
    seg = torch.empty((int(fb[-1]) * n, 8 + S), dtype=torch.uint8, device="cuda")
    for f, c in enumerate(counts):
        if c:
            ctx.fec_encode_packets_device(h, src_arg(src[fb[f]:fb[f + 1]]), int(classes[f]), int(blocks[f]), out=seg[fb[f] * n:fb[f + 1] * n])
    return seg


def expected(ctx, h, n, src, counts, classes, blocks, order):
    seg = per_flow_packets(ctx, h, n, src, counts, classes, blocks)
    perm, flow = wire_order(counts, n, order)
    return seg.index_select(0, torch.from_numpy(perm).cuda()), flow


def flows_call(ctx, h, src, counts, classes, blocks, order, out=None, want_flow_of=True):
    return ctx.fec_encode_packets_flows_device(h, src_arg(src), begin_of(counts), classes, blocks, order, out=out, want_flow_of=want_flow_of)


def per_flow_values(counts):
    """a different class per flow; block numbers that wrap inside a flow of 6 or more frames (250 + 6 > 255)"""
    nf = len(counts)
    return (1 + 5 * np.arange(nf)) & 0xFF, (250 + 37 * np.arange(nf)) & 0xFF


# ------------------------------------------------------------------------------------------ contexts and codes
class Variants:
    """One context per variant -- "default", "words" (symbol unit 4), "nopkt" (LDPC_AMD_ENC_PKT=0) -- and their code handles."""

    def __init__(self):
        self.ctx, self.codes = {}, {}

    def get(self, variant, which):
        if variant not in self.ctx:
            c = api.Context(0)
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            if variant == "words":
                c.set_symbol_unit(4)
            if variant == "nopkt":
                c.configure("LDPC_AMD_ENC_PKT", 0)
            self.ctx[variant] = c
        c = self.ctx[variant]
        if (variant, which) not in self.codes:
            if which == "heavy":
                code = heavy_code()
                self.codes[variant, which] = (c.register_code(code), code)
            else:
                self.codes[variant, which] = (c.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which]), codes.load_builtin(which))
        return (c,) + self.codes[variant, which]

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def variants():
    v = Variants()
    yield v
    v.close()


@pytest.fixture(scope="module")
def ctx(variants):
    return variants.get("default", 1)[0]


# ------------------------------------------------------------------------------------------ 1. bytes, flow_of, packet_begin, path
# (variant, code, S, path the header promises)
PATHS = [
    ("default", 1, 1024, "fused"), ("default", 1, 128, "fused"), ("default", 3, 1024, "fused"), ("words", 1, 20, "fused"),
    ("default", 1, 16, "composed"), ("default", 1, 1, "composed"), ("default", "heavy", 128, "composed"), ("nopkt", 1, 1024, "composed"),
]
# one flow (the single-flow call's bytes); unequal lengths with an empty flow and a stride that changes mid-stream; equal flows;
# stride 64 (n * 64 * (8 + S) is above 2^27 for the built-in codes at S = 1024); block numbers that wrap inside a flow (250 + 9, 31 + 7)
SHAPES = [(5,), (2, 0, 5), (3,) * 8, (1,) * 64, (9, 7)]


@pytest.mark.parametrize("variant,which,S,path", PATHS)
def test_packets_equal_the_per_flow_calls_placed_by_the_rounds(variants, variant, which, S, path):
    c, h, code = variants.get(variant, which)
    n = code.n
    for counts in SHAPES:
        F = sum(counts)
        src = make_source(F, code.k, S, seed=300 + 11 * S + F)
        classes, blocks = per_flow_values(counts)
        for order in (SEG, RR):
            want, want_flow = expected(c, h, n, src, counts, classes, blocks, order)
            single = c.fec_sender_info()["path"]
            got, flow_of, pb = flows_call(c, h, src, counts, classes, blocks, order)
            info = c.fec_sender_flows_info()
            c.synchronize()
            assert info["path"] == path and info["frames"] == F, (counts, order, info)
            assert c.fec_sender_info()["path"] == single, "the single-flow info must keep reporting the single-flow call"
            assert tuple(got.shape) == (F * n, 8 + S) and torch.equal(got, want), (counts, order)
            assert flow_of.dtype == torch.int32 and np.array_equal(flow_of.cpu().numpy(), want_flow), (counts, order)
            assert pb.dtype == np.int64 and np.array_equal(pb, begin_of(counts) * n)
            if len(counts) == 1:   # one flow: the single-flow call's array, in either order
                assert torch.equal(got, c.fec_encode_packets_device(h, src_arg(src), int(classes[0]), int(blocks[0])))
    if path == "fused":
        assert "ldpc_scatter_static_flw_kernel" in c.profile_kernel_names()["apply"]


@pytest.mark.parametrize("S,path", [(128, "fused"), (16, "composed")])
def test_packets_equal_oracle_built_packets(variants, oracle, S, path):
    c, h, code = variants.get("default", 1)
    n, counts = code.n, (2, 0, 5)
    classes, blocks = per_flow_values(counts)
    fb = begin_of(counts)
    src = make_source(sum(counts), code.k, S, seed=77 + S)
    src_h = src.cpu().numpy()
    seg = np.concatenate([oracle_packets(oracle, code, src_h[fb[f]:fb[f + 1]], int(classes[f]), int(blocks[f]))
                          for f in range(len(counts)) if counts[f]])
    for order in (SEG, RR):
        perm, flow = wire_order(counts, n, order)
        got, flow_of, _ = flows_call(c, h, src, counts, classes, blocks, order)
        assert c.fec_sender_flows_info()["path"] == path
        c.synchronize()
        assert np.array_equal(got.cpu().numpy(), seg[perm]), order
        assert np.array_equal(flow_of.cpu().numpy(), flow), order


# ------------------------------------------------------------------------------------------ 2. guard bands
@pytest.mark.parametrize("order", [SEG, RR])
def test_guard_bands_at_three_alignments(ctx, variants, order):
    _, h, code = variants.get("default", 1)
    n, S, counts, G = code.n, 128, (2, 0, 5), 4096
    F = sum(counts)
    classes, blocks = per_flow_values(counts)
    src = make_source(F, code.k, S, seed=41)
    want, want_flow = expected(ctx, h, n, src, counts, classes, blocks, order)
    want_h = want.cpu().numpy()
    nbytes = F * n * (8 + S)
    for shift, must_be in ((0, "fused"), (8, "fused"), (1, "composed")):
        big = torch.full((G + 16 + nbytes + G + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        start = G + (-(big.data_ptr() + G) % 16) + shift              # 16-byte aligned, then + shift
        assert (big.data_ptr() + start) % 16 == shift
        big[start:start + nbytes] = 0x5A
        out = big[start:start + nbytes].view(F * n, 8 + S)
        fbig = torch.full((1024 + F * n + 1024,), -7, dtype=torch.int32, device="cuda")
        L = ctx._L
        fb, cls, blk = begin_of(counts), classes.astype(np.uint8), blocks.astype(np.uint8)
        rc = L.ldpc_amd_fec_encode_packets_flows_dev(ctx._h, h, S, len(counts), fb.ctypes.data, src.data_ptr(), cls.ctypes.data, blk.ctypes.data,
                                                     order, out.data_ptr(), fbig.data_ptr() + 4 * 1024, None)
        assert rc == 0, L.ldpc_amd_last_error(ctx._h)
        path = ctx.fec_sender_flows_info()["path"]
        ctx.synchronize()
        assert path == must_be, (shift, path)
        host = big.cpu().numpy()
        assert (host[:start] == 0xA5).all() and (host[start + nbytes:] == 0xA5).all(), f"guard band touched at shift {shift} ({path})"
        assert np.array_equal(host[start:start + nbytes].reshape(F * n, 8 + S), want_h), (shift, path)   # every byte inside written
        fh = fbig.cpu().numpy()
        assert (fh[:1024] == -7).all() and (fh[1024 + F * n:] == -7).all() and np.array_equal(fh[1024:1024 + F * n], want_flow)


# ------------------------------------------------------------------------------------------ 3. the first packet array beyond 2^32 bytes
def test_round_robin_across_the_32_bit_edge(ctx, variants):
    """2041 frames of (2040,1530) at S = 1024: 2040 * 1032 * 2041 bytes is the first packet array above 2^32.  Compared on the
    device; about 13 GB of device memory at the peak, no host copy of the array."""
    _, h, code = variants.get("default", 1)
    n, S = code.n, 1024
    counts = (400, 13, 301, 255, 256, 257, 500, 59)
    F = sum(counts)
    assert F == 2041 and n * (8 + S) * (F - 1) < 1 << 32 <= n * (8 + S) * F
    classes, blocks = per_flow_values(counts)
    src = make_source(F, code.k, S, seed=9)
    seg = per_flow_packets(ctx, h, n, src, counts, classes, blocks)
    got, flow_of, _ = flows_call(ctx, h, src, counts, classes, blocks, RR)
    assert ctx.fec_sender_flows_info()["path"] == "fused"
    ctx.synchronize()
    del src
    perm, flow = wire_order(counts, n, RR)
    want = seg.index_select(0, torch.from_numpy(perm).cuda())
    del seg
    assert torch.equal(got, want)
    assert torch.equal(flow_of, torch.from_numpy(flow).cuda())
    del got, want
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ 4. the path is the one promised
def test_path_reports_and_fused_equals_composed():
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        assert c.fec_sender_flows_info() == {"path": "none", "scratch_bytes": 0, "descriptor_bytes": 0, "frames": 0}
        h = c.load_builtin_code(1, codes.DEFAULT_COEF_SEED[1])
        n, k, _ = c.code_info(h)
        counts = (3, 1, 0, 4)
        classes, blocks = per_flow_values(counts)
        src = make_source(sum(counts), k, 1024, seed=5)
        fused = [flows_call(c, h, src, counts, classes, blocks, order) for order in (SEG, RR)]
        info = c.fec_sender_flows_info()
        assert info["path"] == "fused" and info["frames"] == 8 and info["descriptor_bytes"] > 0
        assert info["scratch_bytes"] == 0                          # a fused-only sequence holds no codeword scratch
        assert c.fec_sender_info() == {"path": "none", "scratch_bytes": 0}   # no single-flow call yet
        assert "ldpc_scatter_static_flw_kernel" in c.profile_kernel_names()["apply"]
        c.configure("LDPC_AMD_ENC_PKT", 0)
        composed = [flows_call(c, h, src, counts, classes, blocks, order) for order in (SEG, RR)]
        info = c.fec_sender_flows_info()
        assert info["path"] == "composed" and 0 < info["scratch_bytes"] <= 256 * MIB
        c.synchronize()
        for a, b in zip(fused, composed):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        c.configure("LDPC_AMD_ENC_PKT", None)
        flows_call(c, h, src, counts, classes, blocks, RR)
        assert c.fec_sender_flows_info()["path"] == "fused"
        # S = 1 is composed whatever the knob says
        flows_call(c, h, make_source(8, k, 1, seed=6), counts, classes, blocks, RR)
        assert c.fec_sender_flows_info()["path"] == "composed"
        c.synchronize()


# ------------------------------------------------------------------------------------------ 5. back to back
@pytest.mark.parametrize("S", [128, 16])
def test_calls_enqueued_back_to_back(ctx, variants, S):
    """Three calls with different frame_begin, no synchronisation in between: each call's descriptors must be the ones its kernels
    read (the third call reuses the staging of the first)."""
    _, h, code = variants.get("default", 1)
    n = code.n
    shapes = [(2, 0, 5), (4, 3), (1,) * 9]
    srcs = [make_source(sum(cn), code.k, S, seed=90 + i) for i, cn in enumerate(shapes)]
    vals = [per_flow_values(cn) for cn in shapes]
    want = [expected(ctx, h, n, s, cn, v[0], v[1], RR) for s, cn, v in zip(srcs, shapes, vals)]
    ctx.synchronize()
    got = [flows_call(ctx, h, s, cn, v[0], v[1], RR) for s, cn, v in zip(srcs, shapes, vals)]   # enqueued without waiting
    ctx.synchronize()
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g[0], w[0]), f"call {i}"
        assert np.array_equal(g[1].cpu().numpy(), w[1]), f"call {i}"


# ------------------------------------------------------------------------------------------ 6. round trip through FecRxFlows
def test_round_trip_through_a_lossy_wire(ctx, variants):
    _, h, code = variants.get("default", 1)
    n, k, S, nf, per = code.n, code.k, 128, 8, 6
    counts = (per,) * nf
    block0 = (250 + 37 * np.arange(nf)) & 0xFF
    src = make_source(nf * per, k, S, seed=31)
    tx = ctx.fec_tx_flows(h, S, nf, fec_class=1, block0=block0)
    pk, flow_of, pb = tx.send(src, begin_of(counts), RR)
    assert np.array_equal(tx.next_block, (block0 + per) & 0xFF)
    keep = torch.rand(pk.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(32)) >= 0.10
    pk, flow_of = pk[keep].contiguous(), flow_of[keep].contiguous()
    rx = ctx.fec_rx_flows(nf, n, k, S)
    closes, blocks, fr, consumed, offered = rx.decode_mixed(h, pk, flow_of, per + 2)
    ctx.synchronize()
    assert np.array_equal(consumed, offered) and int(offered.sum()) == pk.shape[0]
    src_h = src.cpu().numpy().reshape(nf, per, k, S)
    out, st = fr.out.cpu().numpy(), fr.status.cpu().numpy()
    good = total = 0
    base = 0
    for f in range(nf):
        got_blocks = [int(b) for b in blocks[base:base + closes[f]]]
        frames = [(out[base + i], st[base + i]) for i in range(closes[f])]
        base += closes[f]
        while True:
            r = rx.decode_flush(f, h)
            if r is None:
                break
            ctx.synchronize()
            got_blocks.append(int(r[0]))
            frames.append((r[1].out.cpu().numpy()[0], r[1].status.cpu().numpy()[0]))
        assert got_blocks == [int(block0[f] + i) & 0xFF for i in range(per)], f"flow {f}: its own numbering, in order"
        for i, (o, s) in enumerate(frames):
            total += 1
            if s in (api.ST_MP_DONE, api.ST_ML_SOLVED):
                assert np.array_equal(o[:k].reshape(k, S), src_h[f, i]), f"flow {f} block {i}: decodable but not the transmitted source"
                good += 1
    rx.close()
    assert total == nf * per and good >= total // 2


# ------------------------------------------------------------------------------------------ 7. FecTxFlows
def test_fec_tx_flows_numbers_blocks_across_calls(ctx, variants):
    _, h, code = variants.get("default", 1)
    n, S, nf = code.n, 16, 3
    block0, classes = np.array([250, 0, 255]), np.array([1, 0xAB, 7])
    parts = [(3, 0, 2), (4, 1, 0), (2, 2, 1)]                       # frames of each flow in each of three sends
    total = np.sum(parts, axis=0)
    srcs = [make_source(int(sum(p)), code.k, S, seed=120 + i) for i, p in enumerate(parts)]
    tx = ctx.fec_tx_flows(h, S, nf, fec_class=classes, block0=block0)
    assert np.array_equal(tx.next_block, block0)
    sent = [tx.send(s, begin_of(p), SEG) for s, p in zip(srcs, parts)]
    assert np.array_equal(tx.next_block, (block0 + total) & 0xFF)  # 250 + 9 wraps
    # one call over the concatenation, per flow: flow f's frames of the three sends in a row
    per_flow_src = [torch.cat([s[begin_of(p)[f]:begin_of(p)[f + 1]] for s, p in zip(srcs, parts)]) for f in range(nf)]
    whole, _, wb = flows_call(ctx, h, torch.cat(per_flow_src), tuple(int(t) for t in total), classes, block0, SEG)
    ctx.synchronize()
    for f in range(nf):
        mine = torch.cat([pk[pb[f]:pb[f + 1]] for (pk, _, pb) in sent])
        assert torch.equal(mine, whole[wb[f]:wb[f + 1]]), f"flow {f}"


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_context_usable(ctx, variants):
    L = api.load_library()
    _, h, code = variants.get("default", 1)
    n, k, S, counts = code.n, code.k, 16, (1, 0, 2)
    F, nf = sum(counts), len(counts)
    classes, blocks = per_flow_values(counts)
    cls, blk, fb = classes.astype(np.uint8), blocks.astype(np.uint8), begin_of(counts)
    src_d = make_source(F, k, S, seed=80)
    pk_d = torch.full((F * n, 8 + S), 0x5A, dtype=torch.uint8, device="cuda")
    fo_d = torch.zeros(F * n + 4, dtype=torch.int32, device="cuda")
    good = flows_call(ctx, h, src_d, counts, classes, blocks, RR)[0].clone()
    ctx.synchronize()
    call = L.ldpc_amd_fec_encode_packets_flows_dev

    def refused(want, text=None, *, code_h=h, S_=S, nflows=nf, fb_=fb, src=None, cls_=cls, blk_=blk, order=RR, pk=None, fo=None):
        p = lambda a: None if a is None else a.ctypes.data
        rc = call(ctx._h, code_h, S_, nflows, p(fb_), src_d.data_ptr() if src is None else src, p(cls_), p(blk_), order,
                  pk_d.data_ptr() if pk is None else pk, fo_d.data_ptr() if fo is None else fo, None)
        assert rc == want, (rc, want, text)
        msg = L.ldpc_amd_last_error(ctx._h)
        assert msg and (text is None or text in msg), msg
        again = flows_call(ctx, h, src_d, counts, classes, blocks, RR)[0]   # the context is still usable
        ctx.synchronize()
        assert torch.equal(again, good)

    refused(EINVAL, b"nflows", nflows=0)
    refused(EINVAL, b"nflows", nflows=4097, fb_=np.zeros(4098, dtype=np.int64))
    refused(EINVAL, b"null", fb_=None)
    refused(EINVAL, b"null", cls_=None)
    refused(EINVAL, b"null", blk_=None)
    refused(EINVAL, b"start at 0", fb_=np.array([1, 1, 1, 3], dtype=np.int64))
    refused(EINVAL, b"decreases", fb_=np.array([0, 2, 1, 3], dtype=np.int64))
    refused(EINVAL, b"2^31", fb_=np.array([0, 1 << 20, 1 << 20, 1 << 21], dtype=np.int64))   # 2^21 frames of 2040 packets
    refused(EINVAL, b"order", order=2)
    src_h = np.zeros((F, k, S), dtype=np.uint8)
    pk_h = np.zeros((F * n, 8 + S), dtype=np.uint8)
    fo_h = np.zeros(F * n, dtype=np.int32)
    refused(EINVAL, b"device pointers", src=src_h.ctypes.data)
    refused(EINVAL, b"device pointers", pk=pk_h.ctypes.data)
    refused(EINVAL, b"device pointers", fo=fo_h.ctypes.data)
    refused(EINVAL, b"4-byte aligned", fo=fo_d.data_ptr() + 2)
    both = torch.zeros(F * k * S + F * n * (8 + S) + 4 * F * n, dtype=torch.uint8, device="cuda")
    refused(EINVAL, b"overlap", src=both.data_ptr(), pk=both.data_ptr() + F * k * S - 16)
    refused(EINVAL, b"overlap", src=both.data_ptr() + 64, pk=both.data_ptr())
    refused(EINVAL, b"overlap", src=both.data_ptr(), fo=both.data_ptr() + F * k * S - 16)                     # flow_of in the source
    refused(EINVAL, b"overlap", pk=both.data_ptr(), fo=both.data_ptr() + F * n * (8 + S) - 16)                # flow_of in the packets
    src24 = torch.zeros((F, k, 24), dtype=torch.uint8, device="cuda")
    pk24 = torch.zeros((F * n, 8 + 24), dtype=torch.uint8, device="cuda")
    refused(EUNSUP, b"multiple of 16", S_=24, src=src24.data_ptr(), pk=pk24.data_ptr())
    nt = non_triangular_code()
    hnt = ctx.register_code(nt)
    src_nt = torch.zeros((F, nt.k, S), dtype=torch.uint8, device="cuda")
    pk_nt = torch.zeros((F * nt.n, 8 + S), dtype=torch.uint8, device="cuda")
    refused(EUNSUP, b"triangle form", code_h=hnt, src=src_nt.data_ptr(), pk=pk_nt.data_ptr())
    refused(ENOCODE, b"unknown code handle", code_h=999)
    # word-sized symbols: the source must be 4-byte aligned
    cw, hw, _ = variants.get("words", 1)
    s20 = torch.zeros(F * k * 20 + 4, dtype=torch.uint8, device="cuda")
    p20 = torch.zeros((F * n, 8 + 20), dtype=torch.uint8, device="cuda")
    assert call(cw._h, hw, 20, nf, fb.ctypes.data, s20.data_ptr() + 1, cls.ctypes.data, blk.ctypes.data, RR, p20.data_ptr(), None, None) == EINVAL
    assert b"4-byte aligned" in L.ldpc_amd_last_error(cw._h)
    assert call(cw._h, hw, 20, nf, fb.ctypes.data, s20.data_ptr(), cls.ctypes.data, blk.ctypes.data, RR, p20.data_ptr(), None, None) == 0
    cw.synchronize()
    # F = 0: OK, and nothing is touched (not even looked at: null pointers pass); an all-empty call through the binding
    pk_d.fill_(0x5A)
    fb0 = np.zeros(nf + 1, dtype=np.int64)
    pb = np.full(nf + 1, -3, dtype=np.int64)
    assert call(ctx._h, h, S, nf, fb0.ctypes.data, None, cls.ctypes.data, blk.ctypes.data, RR, None, None, pb.ctypes.data) == 0
    assert call(ctx._h, h, S, nf, fb0.ctypes.data, src_d.data_ptr(), cls.ctypes.data, blk.ctypes.data, RR, pk_d.data_ptr(), fo_d.data_ptr(), None) == 0
    ctx.synchronize()
    assert bool((pk_d == 0x5A).all()) and (pb == -3).all()
    e_pk, e_fo, e_pb = ctx.fec_encode_packets_flows_device(h, src_d[:0], fb0, classes, blocks, RR)
    assert tuple(e_pk.shape) == (0, 8 + S) and e_fo.numel() == 0 and not e_pb.any()
