"""GPU tests of interleaving depth on the multi-flow wire (include/ldpc_erasure_amd_interleave_flows.h): the windowed multi-flow
receiver created with a depth (rxw_scan_flows_grouped, csrc/rx_window_flows_dev.hip) and the multi-flow sender with a depth
(csrc/wire_dev.hip).

The expected values never come from the code under test: one api.FecRxWindowHost(depth = D) per flow over the same calls
(tests/rxw_flows_depth_cases.py: HostFlowsDepth), tools/flow_mix.py for the mixed calls, the brute-force multiplexer of
tools/interleave_model.py placing every flow's straight single-flow packets for the sender, and the CPU oracle for decoded frames.
tests/test_rxw_flows_depth_cases_cpu.py shows that the streams hold the cases they are meant to, and that the plain rule differs
from the depth-D rule on every one of them."""
import ctypes as C

import numpy as np
import pytest

import interleave_cases as ic
import rxw_cases as rc
import rxw_flows_cases as fc
import rxw_flows_depth_cases as dc
import rxw_flows_mixed_cases as mc
from ldpc_erasure_codes_amd import api, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_interleave import SENDER, Variants, guarded, make_source  # noqa: E402
from test_gpu_rx_window import oracle_frames  # noqa: E402
from test_gpu_rxw_flows import NAMES, dev, dev_at, raw_flush, raw_push, same_flows, same_flush, same_frames, same_push, to_host  # noqa: E402
from test_gpu_rxw_flows_mixed import dev_i32, raw_push_mixed, same_mixed  # noqa: E402

fm, im, wm = mc.fm, ic.im, rc.wm
N, K, S0 = rc.N, rc.K, rc.S
EINVAL = -1
SEG, RR = api.TX_SEGMENTED, api.TX_ROUND_ROBIN
MIB = 1 << 20


@pytest.fixture(scope="module")
def variants():
    v = Variants()
    yield v
    v.close()


@pytest.fixture(scope="module")
def ctx(variants):
    return variants.get("default", "rand")[0]


def flush_split(nflows):
    """(a non-ascending subset, the rest) of the flows."""
    sub = list(range(nflows))[::-2]
    return sub, [f for f in range(nflows) if f not in sub]


# ------------------------------------------------------------------------------------------------------ 1. lockstep
@pytest.mark.parametrize("A", dc.AHEAD)
@pytest.mark.parametrize("W,D", dc.LOCKSTEP_WD)
@pytest.mark.parametrize("nflows", dc.LOCKSTEP_NFLOWS)
def test_lockstep_with_host_objects(ctx, nflows, W, D, A):
    """Every flow against a depth-D host object of its own over calls cut at per-flow random sizes with max_blocks_per_flow from
    (1, 2, 64): after every call closes, blocks (slot order), bytes, flags, consumed, and per flow totals, state and dropped, and the
    pending count; then flush_many on a non-ascending subset and on the rest."""
    streams = dc.lockstep_streams(nflows, W, D, A)
    ncalls = closed = 0
    with ctx.fec_rx_window_flows(nflows, N, K, S0, W, A, depth=D) as rx, dc.HostFlowsDepth(nflows, W, A, D) as hx:
        assert rx.depth == D
        for call in fc.lockstep_calls(hx, streams, dc.lockstep_seed(nflows, W, A, D)):
            pk, fb = fc.concat(call.pieces)
            tag = (nflows, W, D, A, ncalls, call.mb)
            same_push(raw_push(rx, dev(pk), fb, call.mb), call, tag)
            same_flows(rx, hx, tag)
            assert rx.pending().blocks == sum(hx.pending()), tag
            ncalls += 1
            closed += int(call.closes.sum())
        sub, rest = flush_split(nflows)
        closed += same_flush(rx, hx, sub, "flush of a subset")
        same_flows(rx, hx, "flush of a subset")
        if rest:
            closed += same_flush(rx, hx, rest, "flush of the rest")
            same_flows(rx, hx, "flush of the rest")
        assert rx.pending().blocks == 0 and same_flush(rx, hx, None, "second flush") == 0
    assert closed >= nflows - (nflows > 2) and ncalls >= 8


# ------------------------------------------------------------------------------------------------------ 2. mixed calls
@pytest.mark.parametrize("W,D", dc.LOCKSTEP_WD)
@pytest.mark.parametrize("nflows", [3, 70])
def test_mixed_segmented_and_flush_calls_on_one_object(ctx, nflows, W, D):
    """The lockstep schedule with the calls merged at random (tools/flow_mix.py: pattern and unrouted flow numbers by the call's
    number), every third call segmented, and a flush of a subset in the middle of the stream: closes, blocks, bytes, flags, consumed,
    offered, left, the unrouted count and every flow's totals and state equal the host objects' on the packets sorted by flow."""
    A = 10
    streams = dc.lockstep_streams(nflows, W, D, A)
    seed = dc.lockstep_seed(nflows, W, A, D) + 1
    unrouted = left_ones = mixed_calls = flushed = 0
    with ctx.fec_rx_window_flows(nflows, N, K, S0, W, A, depth=D) as rx, dc.HostFlowsDepth(nflows, W, A, D) as hx:
        for i, call in enumerate(fc.lockstep_calls(hx, streams, seed)):
            tag = (nflows, W, D, i, call.mb)
            if i % 3 == 2:
                pk, fb = fc.concat(call.pieces)
                same_push(raw_push(rx, dev(pk), fb, call.mb), call, tag)
            else:
                pk, flow_of = mc.mixed_call(call, i, seed)
                got = raw_push_mixed(rx, dev(pk), dev_i32(flow_of), call.mb)
                same_mixed(rx, got, call, flow_of, tag)
                unrouted += mc.unrouted_in(flow_of, nflows)
                left_ones += int(got[2].sum())
                mixed_calls += 1
            assert rx.unrouted == unrouted, tag
            same_flows(rx, hx, tag)
            if i == 12:   # in the middle of the streams: the flushed flows re-anchor on what comes next
                flushed = same_flush(rx, hx, flush_split(nflows)[0], "flush in the middle")
                same_flows(rx, hx, "flush in the middle")
        assert flushed >= 1 and rx.pending().blocks == sum(hx.pending())
        same_flush(rx, hx, None, "flush")
        same_flows(rx, hx, "flush")
        assert rx.unrouted == unrouted
    assert mixed_calls >= 6 and unrouted > 0 and left_ones > 0


# ------------------------------------------------------------------------------------------------------ 3. depth 1
class ViaCreateDepth(api.FecRxWindowFlows):
    """An object made by ldpc_amd_fec_rxw_flows_create_depth whatever the depth (the class takes the plain create call at depth 1)."""

    def __init__(self, ctx, nflows, n, k, S, window, ahead_limit, depth):
        self._ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        ctx._check(self._L.ldpc_amd_fec_rxw_flows_create_depth(ctx._h, nflows, n, k, S, window, ahead_limit, depth, C.byref(h)), "fec_rxw_flows_create")
        self._h, self.nflows, self.n, self.k, self.S, self.window, self.ahead_limit = h, nflows, n, k, S, window, ahead_limit


def test_depth_1_is_the_plain_object(ctx):
    """create_depth(.., 1) against create on a lockstep stream of tests/rxw_flows_cases.py, and both against the plain host objects:
    byte for byte, segmented and mixed calls."""
    nflows, W, A = 3, 4, 10
    streams = fc.lockstep_streams(nflows, A)
    with ViaCreateDepth(ctx, nflows, N, K, S0, W, A, 1) as r1, ctx.fec_rx_window_flows(nflows, N, K, S0, W, A) as r0, fc.HostFlows(nflows, W, A) as hx:
        assert r1.depth == 1 and r0.depth == 1
        for i, call in enumerate(fc.lockstep_calls(hx, streams, 321)):
            if i & 1:
                pk, flow_of = mc.mixed_call(call, i, 321)
                d_pk, d_fo = dev(pk), dev_i32(flow_of)
                g1, g0 = raw_push_mixed(r1, d_pk, d_fo, call.mb), raw_push_mixed(r0, d_pk, d_fo, call.mb)
                same_mixed(r1, g1, call, flow_of, i)
                for a, b in zip(g1[0] + g1[1:], g0[0] + g0[1:]):
                    assert np.array_equal(a, b), i
            else:
                pk, fb = fc.concat(call.pieces)
                d_pk = dev(pk)
                g1, g0 = raw_push(r1, d_pk, fb, call.mb), raw_push(r0, d_pk, fb, call.mb)
                same_push(g1, call, i)
                for a, b in zip(g1, g0):
                    assert np.array_equal(a, b), i
            same_flows(r1, hx, i)
            same_flows(r0, hx, i)
        assert same_flush(r1, hx, None, "flush") >= nflows
    for D in (2, 8):
        with ViaCreateDepth(ctx, 2, N, K, S0, 16, A, D) as rx, ctx.fec_rx_window_flows(2, N, K, S0, 16, A, depth=D) as ry:
            assert rx.depth == ry.depth == D


# ------------------------------------------------------------------------------------------------------ 4. data paths
def coded_streams(c, h, code, S, counts, D, seed, loss=0.08, **link):
    """Per flow: F random frames through the interleaved single-flow sender on the device, thinned and sent through
    tools/link_model.py's link on the host: packets uint8 [P][8 + S] (numpy)."""
    streams = []
    for f, F in enumerate(counts):
        pk = c.fec_encode_packets_interleaved_device(h, make_source(F, code.k, S, seed + 10 * f), D, 1, (248 + 2 * f) & 0xFF).cpu().numpy()
        keep = np.random.default_rng(seed + 10 * f + 1).random(pk.shape[0]) >= loss
        streams.append(rc.through_link(pk[keep], seed + 10 * f + 2, **link))
    return streams


def decode_four_ways(c, h, code, S, streams, W, A, D, odd=False, mb=3, sizes=(700, 2500, 10 ** 9)):
    """Four depth-D objects over the same calls: decode_many; push_many + Context.decode_frames; decode_mixed on the pieces merged
    at random with unrouted packets; push_mixed + decode_frames.  Everything the calls return must be equal; the end by
    decode_flush_many against flush_many + decode_frames.  Returns (blocks closed, the paths decode_many / decode_mixed reported, the
    flush's)."""
    nf = len(streams)
    pos, paths, closed, i = [0] * nf, set(), 0, 0
    mk = lambda: c.fec_rx_window_flows(nf, code.n, code.k, S, W, A, depth=D)   # noqa: E731
    with mk() as rd, mk() as rp, mk() as md, mk() as mp:
        while any(pos[f] < streams[f].shape[0] for f in range(nf)):
            pieces = [streams[f][pos[f]:pos[f] + sizes[(i + f) % len(sizes)]] for f in range(nf)]
            pk, fb = fc.concat(pieces, S)
            d_pk = dev_at(pk, odd)
            c1, b1, fr, u1 = rd.decode_many(h, d_pk, fb, mb)
            info = c.fec_rx_window_flows_info()
            c0, b0, sym, er, u0 = rp.push_many(d_pk, fb, mb)
            assert np.array_equal(c0, c1) and np.array_equal(b0, b1) and np.array_equal(u0, u1) and u0.sum() > 0, i
            assert info["blocks"] == len(b1)
            paths.add(info["path"])
            mix, flow_of = fm.mix(pieces, fm.PATTERNS[i % len(fm.PATTERNS)], 77 + i, unrouted=True, run=300)
            d_mix, d_fo = dev_at(mix, odd), dev_i32(flow_of)
            c2, b2, fr2, u2, o2, l2 = md.decode_mixed(h, d_mix, d_fo, mb, want_left=True)
            paths.add(c.fec_rx_window_flows_info()["path"])
            c3, b3, sym3, er3, u3, o3, l3 = mp.push_mixed(d_mix, d_fo, mb, want_left=True)
            for cc, bb, uu in ((c2, b2, u2), (c3, b3, u3)):
                assert np.array_equal(cc, c1) and np.array_equal(bb, b1) and np.array_equal(uu, u1), i
            assert np.array_equal(o2, np.diff(fb)) and np.array_equal(o3, o2), i
            want_left = fm.left_model(flow_of, nf, u1)
            assert np.array_equal(l2.cpu().numpy(), want_left) and torch.equal(l2, l3), i
            assert torch.equal(sym3, sym) and torch.equal(er3, er), i
            if len(b1):
                want = to_host(c.decode_frames(h, sym, er), S)
                same_frames(to_host(fr, S), want, ("decode_many", i))
                same_frames(to_host(fr2, S), want, ("decode_mixed", i))
                assert info["launches"] >= 1
            for f in range(nf):
                pos[f] += int(u1[f])
            closed += len(b1)
            i += 1
        assert md.unrouted == mp.unrouted > 0 and rd.unrouted == 0
        order = list(range(nf))[::-1]
        assert rd.pending().blocks == rp.pending().blocks == md.pending().blocks >= 1
        c1, b1, fr = rd.decode_flush_many(h, order)
        finfo = c.fec_rx_window_flows_info()
        c0, b0, sym, er = rp.flush_many(order)
        c2, b2, fr2 = md.decode_flush_many(h, order)
        c3, b3, sym3, er3 = mp.flush_many(order)
        assert np.array_equal(c0, c1) and np.array_equal(b0, b1) and np.array_equal(c2, c1) and np.array_equal(b2, b1) and len(b0) >= 1
        assert np.array_equal(c3, c1) and np.array_equal(b3, b1) and torch.equal(sym3, sym) and torch.equal(er3, er)
        want = to_host(c.decode_frames(h, sym, er), S)
        same_frames(to_host(fr, S), want, "decode_flush_many")
        same_frames(to_host(fr2, S), want, "decode_flush_many behind mixed calls")
        for f in range(nf):
            assert rd.stats(f) == rp.stats(f) == md.stats(f) == mp.stats(f) and rd.state(f) == rp.state(f) == md.state(f)
    return closed + len(b0), paths, finfo["path"]


DATA_PATHS = [("default", "rand", 16, False), ("default", "rand", 16, True), ("default", 1, 128, False), ("default", "rand", 1, False),
              ("words", "rand", 20, False), ("words", "rand", 20, True)]


@pytest.mark.parametrize("variant,which,S,odd", DATA_PATHS)
def test_decode_many_equals_push_many_and_decode_frames(variants, variant, which, S, odd):
    """Behind the grouped scan of three flows: the 16-byte path and the byte path of the gather and the staging update (S = 1,
    word symbols, a packet array at an odd byte address), the fused and the composed decode (the rx_pkt knob), segmented and mixed."""
    c, h, code = variants.get(variant, which)
    D, W, A = 4, 8, 10
    counts = (10, 7, 9) if which == "rand" else (5, 4, 6)
    assert max(counts) <= 24
    streams = coded_streams(c, h, code, S, counts, D, seed=800 + S, window=code.n // 2, dup=0.02)
    closed, paths, fpath = decode_four_ways(c, h, code, S, streams, W, A, D, odd)
    assert closed >= sum(counts) - 1
    if which == 1:
        assert paths == {"fused"} and fpath == "fused", "built-in code 1 at S = 128, aligned: the packets-in decoder"
    if odd:
        assert paths == {"composed"}
    c.configure("LDPC_AMD_RX_PKT", 0)
    try:
        closed0, paths0, fpath0 = decode_four_ways(c, h, code, S, streams, W, A, D, odd)
    finally:
        c.configure("LDPC_AMD_RX_PKT", None)
    assert closed0 == closed and paths0 == {"composed"} and fpath0 == "composed"


# ------------------------------------------------------------------------------------------------------ 5. the sender
COUNTS = {RR: (8, 0, 16, 8), SEG: (11, 0, 3, 6)}   # whole groups of every depth up to 8 / short first and last runs, an empty flow
SEND_BLOCK0 = {RR: (248, 5, 0, 16), SEG: (250, 7, 255, 13)}
SEND_CLASS = (7, 1, 200, 3)


def begin_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def straight_packets(c, h, n, src, counts, classes, blocks):
    """Every flow's packets from the straight single-flow sender, flow after flow in frame and row order."""
    S = 1 if src.ndim == 2 else src.shape[2]
    fb = begin_of(counts)
    seg = torch.empty((int(fb[-1]) * n, 8 + S), dtype=torch.uint8, device="cuda")
    for f, cnt in enumerate(counts):
        if cnt:
            c.fec_encode_packets_device(h, src[fb[f]:fb[f + 1]], int(classes[f]), int(blocks[f]), out=seg[fb[f] * n:fb[f + 1] * n])
    return seg


def wire_of(counts, n, blocks, D, order):
    """(index into the straight array [P], flow [P]) of every wire position, from the brute-force multiplexer."""
    frame, row, flow = im.flows_order(begin_of(counts), n, blocks, D, order)
    return torch.from_numpy(frame * n + row).cuda(), flow.astype(np.int32)


@pytest.mark.parametrize("variant,which,S,path", SENDER)
def test_sender_puts_every_packet_at_the_layouts_index(variants, variant, which, S, path):
    """Both orders at every depth (round robin: up to the depth the counts are whole groups of): index_select of the flows' straight
    packets by the multiplexer's order, between guard bands; flow_of, packet_begin, the path and the three info calls."""
    c, h, code = variants.get(variant, which)
    n = code.n
    for order in (SEG, RR):
        counts, blocks = COUNTS[order], SEND_BLOCK0[order]
        F = sum(counts)
        src = make_source(F, code.k, S, seed=60 + S + order)
        straight = straight_packets(c, h, n, src, counts, SEND_CLASS, blocks)
        others = lambda: [(i["path"], i["frames"]) for i in (c.fec_sender_flows_info(), c.fec_sender_ilv_info())]   # noqa: E731
        before = others()
        for D in (ic.DEPTHS if order == SEG else (1, 2, 4, 8)):
            buf, out = guarded(F * n, 8 + S)
            got, flow_of, pb = c.fec_encode_packets_flows_interleaved_device(h, src, begin_of(counts), SEND_CLASS, blocks, order, D, out=out)
            info = c.fec_sender_flows_ilv_info()
            assert info["path"] == path and info["frames"] == F and info["descriptor_bytes"] >= 20 * F, (order, D, info)
            assert info["scratch_bytes"] <= 256 * MIB and (path == "fused" or info["scratch_bytes"] > 0)
            idx, flow = wire_of(counts, n, blocks, D, order)
            assert torch.equal(got, straight.index_select(0, idx)), (S, order, D)
            assert bool((buf[:8] == 0xA5).all()) and bool((buf[-8:] == 0xA5).all()), "guard bands"
            assert np.array_equal(flow_of.cpu().numpy(), flow) and np.array_equal(pb, begin_of(counts) * n)
            first, stride = api.fec_tx_flows_ilv_layout(begin_of(counts), n, blocks, D, order)
            t, j = F - 2, n - 1   # the contract, read literally, on one packet
            assert torch.equal(got[int(first[t]) + j * int(stride[t])], straight[t * n + j])
            if D == 1:
                old = c.fec_encode_packets_flows_device(h, src, begin_of(counts), SEND_CLASS, blocks, order)
                assert torch.equal(got, old[0]) and torch.equal(flow_of, old[1]) and np.array_equal(pb, old[2]), "depth 1 is the flows call"
                before = others()
            assert others() == before, "the other info calls keep reporting their own last call"
        got, flow_of, _ = c.fec_encode_packets_flows_interleaved_device(h, src, begin_of(counts), SEND_CLASS, blocks, order, 2, want_flow_of=False)
        assert flow_of is None and torch.equal(got, straight.index_select(0, wire_of(counts, n, blocks, 2, order)[0]))


def test_sender_fused_equals_composed(variants):
    c, h, code = variants.get("default", 1)
    S, counts, blocks = 128, COUNTS[RR], SEND_BLOCK0[RR]
    src = make_source(sum(counts), code.k, S, seed=6)
    call = lambda D, order: c.fec_encode_packets_flows_interleaved_device(h, src, begin_of(counts), 1, blocks, order, D)[0]   # noqa: E731
    fused = [call(D, order) for D in (4, 8) for order in (SEG, RR)]
    assert c.fec_sender_flows_ilv_info()["path"] == "fused"
    c.configure("LDPC_AMD_ENC_PKT", 0)
    try:
        composed = [call(D, order) for D in (4, 8) for order in (SEG, RR)]
        info = c.fec_sender_flows_ilv_info()
    finally:
        c.configure("LDPC_AMD_ENC_PKT", None)
    assert info["path"] == "composed" and 0 < info["scratch_bytes"] <= 256 * MIB
    for a, b in zip(fused, composed):
        assert torch.equal(a, b)


def test_three_senders_back_to_back(variants):
    """The descriptor staging is shared by the three descriptor-driven senders: differently shaped calls of all three enqueued
    without a synchronisation in between, each with another table, are all right, and each reports through its own info."""
    c, h, code = variants.get("default", 1)
    n, S = code.n, 128
    a_src, b_src, c_src = make_source(12, code.k, S, seed=1), make_source(5, code.k, S, seed=2), make_source(9, code.k, S, seed=3)
    a_counts, a_blocks = (4, 8), (252, 8)
    want_a = straight_packets(c, h, n, a_src, a_counts, (1, 2), a_blocks).index_select(0, wire_of(a_counts, n, a_blocks, 4, RR)[0])
    want_b = straight_packets(c, h, n, b_src, (2, 3), (2, 2), (255, 255))
    frame, row = im.order(9, n, 3, 8)
    want_c = c.fec_encode_packets_device(h, c_src, 1, 3).index_select(0, torch.from_numpy(frame * n + row).cuda())
    want_d = straight_packets(c, h, n, a_src, (5, 7), (1, 2), (250, 9)).index_select(0, wire_of((5, 7), n, (250, 9), 8, SEG)[0])
    c.synchronize()
    a = c.fec_encode_packets_flows_interleaved_device(h, a_src, begin_of(a_counts), (1, 2), a_blocks, RR, 4)[0]
    b = c.fec_encode_packets_flows_device(h, b_src, [0, 2, 5], 2, 255, SEG)[0]
    ci = c.fec_encode_packets_interleaved_device(h, c_src, 8, 1, 3)
    d = c.fec_encode_packets_flows_interleaved_device(h, a_src, begin_of((5, 7)), (1, 2), (250, 9), SEG, 8)[0]
    assert c.fec_sender_flows_ilv_info()["frames"] == 12 and c.fec_sender_flows_info()["frames"] == 5 and c.fec_sender_ilv_info()["frames"] == 9
    c.synchronize()
    assert torch.equal(a, want_a) and torch.equal(b, want_b) and torch.equal(ci, want_c) and torch.equal(d, want_d)


# ------------------------------------------------------------------------------------------------------ 6. end to end
E2E_NF, E2E_F, E2E_D, E2E_W, E2E_A = 4, 32, 4, 16, 10
E2E_BLOCK0 = (248, 0, 252, 100)


@pytest.mark.parametrize("window", [0, 64])
def test_end_to_end_sender_link_receiver(ctx, variants, oracle, window):
    """FecTxFlows(depth 4, round robin) -> FecLink (Gilbert-Elliott loss at the cfg 3 parameters by wire position; no reordering /
    reordering within 64 packet times) -> FecRxWindowFlows(depth 4, W = 16, A = 10).decode_mixed and decode_flush_many on the
    (300,200) code: every flow is its FecRxWindowHost(depth 4) fed the same arrivals, and the decoded frames are the oracle's."""
    S = 16
    _, h, code = variants.get("default", "rand")
    n, k = code.n, code.k
    oc = oracle.OracleCode(code)
    src = make_source(E2E_NF * E2E_F, k, S, seed=19)
    tx = ctx.fec_tx_flows(h, S, E2E_NF, block0=E2E_BLOCK0, depth=E2E_D)
    pk, flow_of, _ = tx.send(src, np.arange(E2E_NF + 1) * E2E_F, RR)
    assert tx.next_block.tolist() == [(b + E2E_F) & 0xFF for b in E2E_BLOCK0]
    P = pk.shape[0]
    lost = dev(synth.erasures_bursty(83, 0, P, 1, 0.13, 0.8, 10.0).reshape(-1))
    arrived, fo, _, _ = ctx.fec_link(seed=7, window=window).send(pk, lost, flow_of)
    pk_host, fo_host = arrived.cpu().numpy(), fo.cpu().numpy()
    assert 0 < pk_host.shape[0] < P
    with ctx.fec_rx_window_flows(E2E_NF, n, k, S, E2E_W, E2E_A, depth=E2E_D) as rx, dc.HostFlowsDepth(E2E_NF, E2E_W, E2E_A, E2E_D, S_=S, n=n, k=k) as hx:
        closes, blocks, fr, consumed, offered, left = rx.decode_mixed(h, arrived.contiguous(), fo.contiguous(), 64, want_left=True)
        pieces = [pk_host[fo_host == f] for f in range(E2E_NF)]
        hc, hb, hs, he, hu = hx.push_many(pieces, 64)
        assert np.array_equal(closes, hc) and np.array_equal(blocks, hb) and np.array_equal(consumed, hu)
        assert np.array_equal(offered, [p.shape[0] for p in pieces]) and np.array_equal(consumed, offered) and not bool(left.any())
        same_flows(rx, hx, "decode_mixed")
        fcl, fbl, ffr = rx.decode_flush_many(h)
        hfc, hfb, hfs, hfe = hx.flush_many()
        assert np.array_equal(fcl, hfc) and np.array_equal(fbl, hfb)
        same_flows(rx, hx, "decode_flush_many")
        assert rx.unrouted == 0
    assert len(hb) + len(hfb) >= E2E_NF * (E2E_F - 1)
    for got, sym, er, tag in ((to_host(fr, S), hs, he, "decode_mixed"), (to_host(ffr, S), hfs, hfe, "decode_flush_many")):
        if sym.shape[0]:
            for name, a, w in zip(NAMES[:4], got[:4], oracle_frames(oc, sym, er)):
                assert np.array_equal(a, w), (tag, name)


# ------------------------------------------------------------------------------------------------------ 7. refusals
def test_receiver_refusals_are_atomic(ctx):
    L = ctx._L
    h = C.c_void_p()
    for depth in (0, 3, 32, -2):
        assert L.ldpc_amd_fec_rxw_flows_create_depth(ctx._h, 3, N, K, 16, 32, 10, depth, C.byref(h)) == EINVAL
        assert b"depth" in L.ldpc_amd_last_error(ctx._h) and not h.value
    for W, D in [(3, 2), (7, 4), (31, 16), (16, 16)]:
        assert L.ldpc_amd_fec_rxw_flows_create_depth(ctx._h, 3, N, K, 16, W, 10, D, C.byref(h)) == EINVAL
        assert b"2 * depth <= window" in L.ldpc_amd_last_error(ctx._h) and not h.value
        with pytest.raises(api.LdpcAmdError):
            ctx.fec_rx_window_flows(3, N, K, 16, W, 10, depth=D)
    assert L.ldpc_amd_fec_rxw_flows_create_depth(ctx._h, 0, N, K, 16, 8, 10, 4, C.byref(h)) == EINVAL and b"nflows" in L.ldpc_amd_last_error(ctx._h)
    assert L.ldpc_amd_fec_rxw_flows_create_depth(ctx._h, 3, N, K, 16, 33, 10, 4, C.byref(h)) == EINVAL and b"window" in L.ldpc_amd_last_error(ctx._h)
    nf, W, A, D, mb = 3, 8, 10, 4, 4
    streams = dc.lockstep_streams(nf, W, D, A)
    first, rest = [pk[:1000] for pk in streams], [pk[1000:] for pk in streams]
    with ctx.fec_rx_window_flows(nf, N, K, S0, W, A, depth=D) as rx, dc.HostFlowsDepth(nf, W, A, D) as hx:
        pk, fb = fc.concat(first)
        same_push(raw_push(rx, dev(pk), fb, 64), fc.Call(64, None, first, *hx.push_many(first, 64)), "first")
        before = [(rx.state(f), rx.stats(f)) for f in range(nf)]
        assert sum(sum(s["cnt"]) for s, _ in before) > 0
        pk, fb = fc.concat(rest)
        d_pk = dev(pk)
        sym = torch.empty((nf * mb, N, S0), dtype=torch.uint8, device="cuda")
        er = torch.empty((nf * mb, N), dtype=torch.uint8, device="cuda")
        host = np.zeros((nf * mb, N, S0), dtype=np.uint8)
        closes, used = np.zeros(nf, np.int32), np.zeros(nf, np.int64)

        def push(packets=d_pk.data_ptr(), s=sym.data_ptr(), m=mb):
            return L.ldpc_amd_fec_rxw_flows_push_many(rx._h, packets, fb.ctypes.data, s, er.data_ptr(), None, closes.ctypes.data, m, used.ctypes.data)

        for call, text in [(lambda: push(packets=pk.ctypes.data), b"device pointers"), (lambda: push(s=host.ctypes.data), b"device pointers"),
                           (lambda: push(m=0), b"max_blocks_per_flow")]:
            assert call() == EINVAL and text in L.ldpc_amd_last_error(ctx._h), text
            assert [(rx.state(f), rx.stats(f)) for f in range(nf)] == before, text
        assert rx.depth == D
        same_push(raw_push(rx, d_pk, fb, mb), fc.Call(mb, None, rest, *hx.push_many(rest, mb)), "the next good call")
        same_flows(rx, hx, "the next good call")


def test_sender_refusals_leave_the_objects_unchanged(variants):
    c, h, code = variants.get("default", 1)
    L, n, k, S = c._L, code.n, code.k, 128
    counts = (4, 8)
    fb = begin_of(counts)
    src = make_source(12, k, S, seed=8)
    out = torch.full((12 * n, 8 + S), 0xA5, dtype=torch.uint8, device="cuda")
    host = np.zeros((12 * n, 8 + S), dtype=np.uint8)
    cls = np.array([1, 2], dtype=np.uint8)

    def call(begin=fb, blocks=(4, 252), depth=4, order=RR, o=out.data_ptr(), s=src.data_ptr()):
        b0 = np.array(blocks, dtype=np.uint8)
        return L.ldpc_amd_fec_encode_packets_flows_ilv_dev(c._h, h, S, 2, begin.ctypes.data, s, cls.ctypes.data, b0.ctypes.data, order, o, None, None, depth)

    good = c.fec_encode_packets_flows_interleaved_device(h, src, fb, cls, (4, 252), RR, 4)[0].clone()
    info = c.fec_sender_flows_ilv_info()
    for depth in (0, 3, 32, -4):
        assert call(depth=depth) == EINVAL and b"depth" in L.ldpc_amd_last_error(c._h)
    assert call(blocks=(4, 250)) == EINVAL and b"whole aligned groups" in L.ldpc_amd_last_error(c._h) and b"flow 1" in L.ldpc_amd_last_error(c._h)
    assert call(begin=begin_of((3, 8))) == EINVAL and b"flow 0" in L.ldpc_amd_last_error(c._h)
    assert call(begin=begin_of((6, 6)), blocks=(2, 250)) == EINVAL and b"flow 0" in L.ldpc_amd_last_error(c._h), "the first offending flow"
    assert call(o=host.ctypes.data) == EINVAL and b"device pointers" in L.ldpc_amd_last_error(c._h)
    assert call(s=None) == EINVAL
    assert call(o=src.data_ptr()) == EINVAL and b"overlap" in L.ldpc_amd_last_error(c._h)
    assert call(order=2) == EINVAL and b"order" in L.ldpc_amd_last_error(c._h)
    assert b"fec_encode_packets_flows_ilv_dev" in L.ldpc_amd_last_error(c._h)
    assert call(begin=begin_of((0, 0)), s=None, o=None) == 0, "no frames: nothing to do"
    c.synchronize()
    assert bool((out == 0xA5).all()) and c.fec_sender_flows_ilv_info() == info, "nothing was enqueued and the info keeps the last good call"
    # FecTxFlows: a refused send raises with the C text and leaves the counters where they were
    tx = c.fec_tx_flows(h, S, 2, fec_class=cls, block0=(4, 250), depth=4)
    with pytest.raises(api.LdpcAmdError, match="whole aligned groups"):
        tx.send(src, fb, RR)
    assert tx.next_block.tolist() == [4, 250]
    seg = tx.send(src, fb, SEG)[0]   # SEGMENTED takes part groups
    assert tx.next_block.tolist() == [8, 2]
    assert torch.equal(seg, straight_packets(c, h, n, src, counts, cls, (4, 250)).index_select(0, wire_of(counts, n, (4, 250), 4, SEG)[0]))
    with pytest.raises(api.LdpcAmdError):
        c.fec_tx_flows(h, S, 2, depth=3)
    assert call() == 0
    c.synchronize()
    assert torch.equal(out, good), "a good call after the refusals"
