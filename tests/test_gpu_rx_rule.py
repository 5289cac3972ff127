"""GPU tests of the close rule as a value (include/ldpc_erasure_amd_rx_rule.h) on the two device objects: the ruled plan scans
(rxw_scan_ruled / rxw_scan_grouped_ruled in csrc/rx_window_dev.hip, rxw_scan_flows_ruled / rxw_scan_flows_grouped_ruled in
csrc/rx_window_flows_dev.hip).  Every comparison is byte for byte against the C host object under the same rule
(api.FecRxWindowHost(rule=)), which tests/test_rx_rule_cpu.py ties to the numpy model; decoded frames against Context.decode_frames
on the same blocks; the Reed-Solomon run against the source bytes and the count of blocks the channel left decodable."""
import ctypes as C

import numpy as np
import pytest

import rx_rule_cases as rr
from code_helpers import random_code
from ldpc_erasure_codes_amd import api

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

rc, wm = rr.rc, rr.wm
N, K, S = rr.N, rr.K, rr.S
EINVAL = -1
NAMES = ("out", "sweeps", "residual", "status", "erased_out", "residual_src")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture(scope="module")
def code(ctx):
    """A small registered (200,150) code: the n and k of the streams."""
    cd = random_code(n=N, k=K)
    return ctx.register_code(cd), cd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def lockstep(ctx, pk, W, A, D, rule, calls, end=True):
    """The device object and the host object under one rule over the same calls [(start, end, max_blocks)]; a call that stops early
    is followed by calls over the rest of its piece.  Every call's blocks, bytes, flags, consumed, totals and state must agree; then
    the flushes."""
    d_pk = dev(pk)
    closed = 0
    with ctx.fec_rx_window(N, K, pk.shape[1] - 8, W, A, depth=D, rule=rule) as rx, api.FecRxWindowHost(N, K, pk.shape[1] - 8, W, A, depth=D, rule=rule) as hx:
        assert rx.rule == hx.rule == (tuple(rule) if rule is not None else api.fec_rx_rule_default(N, K)) and rx.depth == D
        for s, e, mb in calls:
            pos = s
            while True:
                hb, hs, he, hu = hx.push_many(pk[pos:e], mb)
                b, sy, er, u = rx.push_many(d_pk[pos:e], mb)
                tag = (W, A, D, rule, s, e, mb, pos)
                assert u == hu and np.array_equal(b, hb), tag
                assert np.array_equal(sy.cpu().numpy(), hs) and np.array_equal(er.cpu().numpy(), he), tag
                assert rx.stats() == hx.stats() and rx.state() == hx.state() and rx.dropped == hx.dropped, tag
                closed += len(b)
                pos += u
                if pos >= e:
                    break
        if end:
            hb, hs, he = hx.flush()
            b, sy, er = rx.flush()
            assert np.array_equal(b, hb) and np.array_equal(sy.cpu().numpy(), hs) and np.array_equal(er.cpu().numpy(), he)
            assert rx.stats() == hx.stats() and rx.state() == hx.state()
            assert len(rx.flush()[0]) == 0
            closed += len(b)
    return closed


def random_calls(P, seed):
    rng = np.random.default_rng(seed)
    calls, pos = [], 0
    while pos < P:
        c = int(rng.choice([1, 17, 63, 64, 65, 300, 1111]))
        calls.append((pos, min(pos + c, P), int(rng.choice([1, 2, 64]))))
        pos += c
    return calls


# ------------------------------------------------------------------------------------------------------ 1. the single-flow object
CONFIGS = [(1, 2, 0), (1, 3, 10), (1, 16, 10), (1, 16, 0), (4, 8, 10)]   # (D, W, A); D = 4: the grouped ruled kernel


@pytest.mark.parametrize("D,W,A", CONFIGS)
@pytest.mark.parametrize("name", rr.RULE_NAMES)
def test_random_streams_under_every_rule(ctx, name, D, W, A):
    """The random streams and the wrap stream in calls of mixed sizes with max_blocks from (1, 2, 64)."""
    rule = rr.rules(D)[name]
    closed = 0
    for seed in rr.RANDOM_SEEDS + ["wrap"]:
        pk = rc.random_stream(**rr.WRAP) if seed == "wrap" else rc.random_stream(seed)
        closed += lockstep(ctx, pk, W, A, D, rule, random_calls(pk.shape[0], 7))
    assert closed >= 13


@pytest.mark.parametrize("A", rr.EDGE_A)
@pytest.mark.parametrize("D,W", rr.EDGE_DEPTH)
def test_mds_plan_edges(ctx, D, W, A):
    """The MDS rule's edge stream in its call cuts: a give-up close of an empty slot 0 (an all-erased block), a give-up close with
    three closes on the packets behind it inside one group of 64, events on lane 0, lane 63 and the last packet of a call, a
    re-anchor under c_lo == 0, the wrap, a call of fewer than 64 packets (tests/test_rx_rule_cpu.py asserts that the stream and
    the cuts do all that); then with max_blocks = 1, every close ending a call in the middle of a cascade; then under the other
    rules."""
    blk, sym = rr.edge_stream(A)
    pk = rc.packets_of(blk, sym)
    calls = rr.edge_calls(blk, sym, W, A, D)
    mds = wm.mds_rule(N, K, D)
    many = [(s, e, 64) for s, e in calls]
    many.insert(2, (calls[2][0], calls[2][0], 1))   # npackets = 0 in the middle of the stream
    assert lockstep(ctx, pk, W, A, D, mds, many) >= 10
    assert lockstep(ctx, pk, W, A, D, mds, [(0, pk.shape[0], 1)]) >= 10
    assert lockstep(ctx, pk, W, A, D, mds, [(0, 777, 2), (777, pk.shape[0], 3)]) >= 10
    for name in ("at_k", "giveup5", "never"):
        lockstep(ctx, pk, W, A, D, rr.rules(D)[name], many)


def test_a_close_on_every_packet_of_a_group(ctx):
    """The close cascade at its longest: under (0, 1, 0, 1) a packet closes a block whenever a later slot holds one.  After one
    packet of block 9, the packets of blocks 40, 41, 42, ... each land in the last slot of the window (W = 32) and each close slot 0,
    so whole groups of 64 packets carry 64 close events (the inner loop's bound)."""
    W, A, rule = 32, 0, (0, 1, 0, 1)
    blk = np.array([9] + list(range(40, 240)), dtype=np.int64)
    sym = np.arange(blk.shape[0]) % N
    ev = wm.events(blk, sym, N, K, W, A, rule=rule)
    assert ev == [(p, "close") for p in range(1, blk.shape[0])], "one close per packet from the second packet on"
    pk = rc.packets_of(blk, sym)
    assert lockstep(ctx, pk, W, A, 1, rule, [(0, pk.shape[0], 64)]) >= 200
    assert lockstep(ctx, pk, W, A, 1, rule, [(0, 70, 256), (70, pk.shape[0], 256)]) >= 200


def to_host(fr, S_):
    r = [x.cpu().numpy() for x in fr]
    r[0] = r[0].reshape(r[0].shape[0], r[4].shape[1], S_)
    return r


def same_frames(got, want, tag):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (tag, name)


def coded_stream(ctx, h, cd, F, seed, block0, D=1, loss=0.1):
    """F random frames encoded and packetised on the device (depth-D order), thinned at random: packets uint8 [P][8 + S] (numpy)."""
    src = torch.randint(0, 256, (F, cd.k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    pk = ctx.fec_encode_packets_interleaved_device(h, src, D, 1, block0).cpu().numpy()
    keep = np.random.default_rng(seed + 1).random(pk.shape[0]) >= loss
    return pk[keep]


@pytest.mark.parametrize("D,W", [(1, 4), (4, 8)])
@pytest.mark.parametrize("name", ["mds", "giveup5", "default"])
def test_decode_many_and_decode_flush_under_a_rule(ctx, code, name, D, W):
    """decode_many == push_many + Context.decode_frames on a second object of the same rule, the blocks are the host object's, and
    decode_flush == flush + decode_frames; most frames decode (the stream is a coded one)."""
    h, cd = code
    rule, A, F = rr.rules(D)[name], 10, 12
    pk = coded_stream(ctx, h, cd, F, 400 + D, 248, D, loss=0.08)
    d_pk = dev(pk)
    host = rr.host_run(pk, W, A, D, rule, flush=True)
    blocks, ok, sizes = [], 0, (700, 900, 10 ** 9)
    with ctx.fec_rx_window(N, K, S, W, A, depth=D, rule=rule) as rx, ctx.fec_rx_window(N, K, S, W, A, depth=D, rule=rule) as ry:
        pos = i = 0
        while pos < pk.shape[0]:
            piece = d_pk[pos:pos + sizes[i % len(sizes)]]
            b, fr, used = rx.decode_many(h, piece, 3)
            b2, sym, er, used2 = ry.push_many(piece, 3)
            assert used == used2 > 0 and np.array_equal(b, b2)
            if len(b):
                same_frames(to_host(fr, S), to_host(ctx.decode_frames(h, sym, er), S), (name, D, pos))
                ok += int((fr.status <= 1).sum().item())
            blocks += b.tolist()
            assert rx.stats() == ry.stats() and rx.state() == ry.state()
            pos += used
            i += 1
        b, fr = rx.decode_flush(h)
        b2, sym, er = ry.flush()
        assert np.array_equal(b, b2)
        if len(b):
            same_frames(to_host(fr, S), to_host(ctx.decode_frames(h, sym, er), S), (name, D, "flush"))
            ok += int((fr.status <= 1).sum().item())
        blocks += b.tolist()
        assert rx.stats() == ry.stats() == host["stats"] and rx.state() == host["state"]
    assert blocks == host["blocks"]
    assert ok >= F // 2, "the wire is in order: whatever the rule, a block has its packets when it is handed out, and most decode"


# ------------------------------------------------------------------------------------------------------ 2. the multi-flow object
class HostFlows:
    """One api.FecRxWindowHost(rule=) per flow."""

    def __init__(self, nflows, W, A, D, rule):
        self.rx = [api.FecRxWindowHost(N, K, S, W, A, depth=D, rule=rule) for _ in range(nflows)]

    def close(self):
        for r in self.rx:
            r.close()

    def push(self, pieces, mb):
        """(closes, blocks, sym, er, consumed) as FecRxWindowFlows.push_many returns them."""
        out = [r.push_many(p, mb) for r, p in zip(self.rx, pieces)]
        return (np.array([len(o[0]) for o in out], dtype=np.int32), np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]),
                np.concatenate([o[2] for o in out]), np.array([o[3] for o in out], dtype=np.int64))

    def flush(self, flows):
        out = [self.rx[f].flush() for f in flows]
        return (np.array([len(o[0]) for o in out], dtype=np.int32), np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]),
                np.concatenate([o[2] for o in out]))


def merged(pieces, nflows, seed):
    """The pieces in one random arrival order that keeps every flow's own order, with a few packets of no flow in between:
    (packets, flow_of int32)."""
    rng = np.random.default_rng(seed)
    extra = rc.packets_of([7] * 9, list(range(9)), seed=seed)
    labels = np.concatenate([np.full(p.shape[0], f, dtype=np.int32) for f, p in enumerate(pieces)] + [np.full(9, nflows + 3, dtype=np.int32)])
    labels = labels[rng.permutation(labels.shape[0])]
    src = list(pieces) + [extra]
    pk = np.zeros((labels.shape[0], 8 + S), dtype=np.uint8)
    for f in range(nflows + 1):
        lab = f if f < nflows else nflows + 3
        pk[labels == lab] = src[f]
    return pk, labels


FLOW_SEEDS = {1: [101], 3: [102, None, 103], 5: [104, 105, None, "wrap", 106]}   # None: a flow that never gets a packet


@pytest.mark.parametrize("D,W", [(1, 4), (4, 8)])
@pytest.mark.parametrize("nflows", [1, 3, 5])
@pytest.mark.parametrize("name", ["mds", "giveup5", "at_k", "never"])
def test_flows_under_a_rule(ctx, code, name, nflows, D, W):
    """Flows of unequal lengths, one of them empty, in alternating segmented and mixed calls with max_blocks_per_flow from (2, 64),
    against one host object per flow: closes, blocks, bytes, flags, consumed, per-flow totals and state; then decode_flush_many of a
    non-ascending list of all flows against the host objects' flushes decoded by Context.decode_frames."""
    h, cd = code
    rule, A = rr.rules(D)[name], 10
    streams = []
    for f, seed in enumerate(FLOW_SEEDS[nflows]):
        pk = np.zeros((0, 8 + S), np.uint8) if seed is None else rc.random_stream(**rr.WRAP) if seed == "wrap" else rc.random_stream(seed)
        streams.append(pk[:pk.shape[0] - 300 * f])
    assert len({s.shape[0] for s in streams}) == nflows
    hx = HostFlows(nflows, W, A, D, rule)
    pos, i, closed = [0] * nflows, 0, 0
    sizes = (300, 64, 1111, 17, 700)
    with ctx.fec_rx_window_flows(nflows, N, K, S, W, A, depth=D, rule=rule) as rx:
        assert rx.rule == tuple(rule) and rx.depth == D
        while any(pos[f] < streams[f].shape[0] for f in range(nflows)):
            pieces = [streams[f][pos[f]:pos[f] + sizes[(i + f) % len(sizes)]] for f in range(nflows)]
            mb = (2, 64)[i % 2]
            want = hx.push(pieces, mb)
            if i % 3 == 1:
                pk, flow_of = merged(pieces, nflows, 50 + i)
                got = rx.push_mixed(dev(pk), dev(flow_of), mb)
                assert np.array_equal(got[5], [p.shape[0] for p in pieces]), "offered"
            else:
                fb = np.concatenate([[0], np.cumsum([p.shape[0] for p in pieces])]).astype(np.int64)
                got = rx.push_many(dev(np.concatenate(pieces)), fb, mb)
            tag = (name, nflows, D, i)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[4], want[4]), tag
            assert np.array_equal(got[2].cpu().numpy(), want[2]) and np.array_equal(got[3].cpu().numpy(), want[3]), tag
            for f in range(nflows):
                assert rx.stats(f) == hx.rx[f].stats() and rx.state(f) == hx.rx[f].state() and rx.dropped(f) == hx.rx[f].dropped, tag + (f,)
                pos[f] += int(want[4][f])
            closed += len(want[1])
            i += 1
        order = list(range(nflows))[::-1]
        closes, blocks, fr = rx.decode_flush_many(h, order)
        wc, wb, wsym, wer = hx.flush(order)
        assert np.array_equal(closes, wc) and np.array_equal(blocks, wb)
        if len(wb):
            same_frames(to_host(fr, S), to_host(ctx.decode_frames(h, dev(wsym), dev(wer)), S), (name, nflows, D, "flush"))
        for f in range(nflows):
            assert rx.stats(f) == hx.rx[f].stats() and rx.state(f) == hx.rx[f].state()
        assert rx.pending().blocks == 0
    hx.close()
    assert closed + len(wb) >= nflows - 1 and i >= 5


# ------------------------------------------------------------------------------------------------------ 3. the default rule
def test_spelled_out_default_rule_gives_the_bytes_of_an_object_without_a_rule(ctx):
    rule = api.fec_rx_rule_default(N, K)
    for D, W, A in [(1, 4, 10), (4, 8, 10)]:
        pk = rc.random_stream(rr.RANDOM_SEEDS[3])
        d_pk = dev(pk)
        with ctx.fec_rx_window(N, K, S, W, A, depth=D) as r0, ctx.fec_rx_window(N, K, S, W, A, depth=D, rule=rule) as r1:
            assert r0.rule == r1.rule == rule
            pos = 0
            while pos < pk.shape[0]:
                a, b = r0.push_many(d_pk[pos:pos + 900], 3), r1.push_many(d_pk[pos:pos + 900], 3)
                assert a[3] == b[3] and np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
                assert r0.stats() == r1.stats() and r0.state() == r1.state()
                pos += a[3]
            a, b = r0.flush(), r1.flush()
            assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and len(a[0]) >= 1
        lockstep(ctx, pk, W, A, D, None, random_calls(pk.shape[0], 3))
        pieces = [pk[:2000], pk[500:1700], pk[:0]]
        fb = np.array([0, 2000, 3200, 3200], dtype=np.int64)
        d_all = dev(np.concatenate(pieces))
        with ctx.fec_rx_window_flows(3, N, K, S, W, A, depth=D) as r0, ctx.fec_rx_window_flows(3, N, K, S, W, A, depth=D, rule=rule) as r1:
            assert r0.rule == r1.rule == rule
            a, b = r0.push_many(d_all, fb, 64), r1.push_many(d_all, fb, 64)
            assert len(a[1]) >= 4
            for x, y in zip(a, b):
                assert torch.equal(x, y) if torch.is_tensor(x) else np.array_equal(x, y)
            a, b = r0.flush_many(), r1.flush_many()
            for x, y in zip(a, b):
                assert torch.equal(x, y) if torch.is_tensor(x) else np.array_equal(x, y)
            for f in range(3):
                assert r0.stats(f) == r1.stats(f) and r0.state(f) == r1.state(f)


# ------------------------------------------------------------------------------------------------------ 4. Reed-Solomon end to end
RS_SEED, RS_BLOCKS, RS_DEPTH = 79, 64, 8
RS_DECODABLE, RS_DEFAULT_DELIVERS = 61, 49   # tools/rx_window_model.py on the trace of seed 79: blocks with k arrived / with k handed out


def test_rs_stream_delivers_every_decodable_block_under_the_mds_rule(ctx):
    """FecTxRs at depth 8, RS(255,192), S = 16, 64 blocks; the packets the CPU's Gilbert-Elliott trace (seed 79, by wire position)
    drops are taken out; FecRxWindow(16, 10, depth = 8, rule = mds).rs_decode_many + rs_decode_flush.  The model says 61 of the 64
    blocks keep k or more packets, and that the default rule hands 49 of them out with k symbols (its forced closes drop 455
    packets ahead of the window).  Under the MDS rule all 61 come back with status OK and their source bytes; under the default
    rule on the same packets fewer do."""
    n, k, D, B = rr.RS_N, rr.RS_K, RS_DEPTH, RS_BLOCKS
    rs = ctx.rs_create(n, k)
    src = torch.randint(0, 256, (B, k, S), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(12))
    pk = ctx.fec_tx_rs(rs, S, depth=D, block0=0).send(src)
    blk, sym, serial = rr.rs_wire(B, D)
    h_blk, h_sym = wm.headers(pk.cpu().numpy())
    assert np.array_equal(h_blk, blk) and np.array_equal(h_sym, sym), "the sender's wire is the one the model was run on"
    keep = rr.burst_keep(RS_SEED, B * n)
    arrived_per_block = np.bincount(serial[keep], minlength=B)
    decodable = set(np.flatnonzero(arrived_per_block >= k).tolist())
    assert len(decodable) == RS_DECODABLE
    arrived = pk[dev(keep)].contiguous()
    src_host = src.cpu().numpy()
    delivered = {}
    for name, rule in (("mds", api.fec_rx_rule_mds(n, k, D)), ("default", None)):
        with ctx.fec_rx_window(n, k, S, 16, 10, depth=D, rule=rule) as rx:
            b1, m1, r1, s1, used = rx.rs_decode_many(rs, arrived, B)
            assert used == arrived.shape[0]
            b2, m2, r2, s2 = rx.rs_decode_flush(rs)
            stats = rx.stats()
        blocks = b1.tolist() + b2.tolist()
        msg, status = torch.cat([m1, m2]).cpu().numpy(), torch.cat([s1, s2]).tolist()
        good = {blocks[j] for j in range(len(blocks)) if status[j] == 0}
        for j in range(len(blocks)):
            if status[j] == 0:
                assert np.array_equal(msg[j], src_host[blocks[j]]), (name, blocks[j])
        print(f"{name}: {len(good)} of {len(decodable)} decodable blocks delivered, totals {stats}")
        delivered[name] = good
        if name == "mds":
            assert stats["ahead_total"] == 0
    assert delivered["mds"] == decodable, "every block with k or more arrived packets comes back with status OK and its source bytes"
    assert len(delivered["default"]) == RS_DEFAULT_DELIVERS < len(delivered["mds"])


# ------------------------------------------------------------------------------------------------------ 5. refusals
BAD = [(-1, 11, 161, 101), (191, -1, 161, 101), (191, 11, -1, 101), (191, 11, 161, -1), (N + 1, 11, 161, 101), (191, 11, N + 1, 101),
       (191, (1 << 30) + 1, 161, 101), (191, 11, 161, (1 << 30) + 1), (0, 0, 161, 101), (191, 11, 0, 0)]


def test_refusals_leave_the_context_usable(ctx):
    L = ctx._L
    for rule in BAD:
        r, h = api.RxRule(*rule), C.c_void_p()
        assert L.ldpc_amd_fec_rxw_dev_create_rule(ctx._h, N, K, S, 4, 10, 1, C.byref(r), C.byref(h)) == EINVAL and not h.value, rule
        assert b"close rule" in L.ldpc_amd_last_error(ctx._h), rule
        assert L.ldpc_amd_fec_rxw_flows_create_rule(ctx._h, 3, N, K, S, 4, 10, 1, C.byref(r), C.byref(h)) == EINVAL and not h.value, rule
        assert b"close rule" in L.ldpc_amd_last_error(ctx._h), rule
        with pytest.raises(api.LdpcAmdError):
            ctx.fec_rx_window(N, K, S, 4, 10, rule=rule)
        with pytest.raises(api.LdpcAmdError):
            ctx.fec_rx_window_flows(2, N, K, S, 4, 10, rule=rule)
    r, h = api.RxRule(K, 1, 0, 75), C.c_void_p()
    assert L.ldpc_amd_fec_rxw_dev_create_rule(ctx._h, N, K, S, 33, 10, 1, C.byref(r), C.byref(h)) == EINVAL and b"window" in L.ldpc_amd_last_error(ctx._h)
    assert L.ldpc_amd_fec_rxw_dev_create_rule(ctx._h, N, K, S, 4, 10, 4, C.byref(r), C.byref(h)) == EINVAL and b"depth" in L.ldpc_amd_last_error(ctx._h)
    assert L.ldpc_amd_fec_rxw_flows_create_rule(ctx._h, 0, N, K, S, 4, 10, 1, C.byref(r), C.byref(h)) == EINVAL and b"nflows" in L.ldpc_amd_last_error(ctx._h)
    assert not h.value
    pk = rc.random_stream(rr.RANDOM_SEEDS[0])
    assert lockstep(ctx, pk, 4, 10, 1, wm.mds_rule(N, K), [(0, pk.shape[0], 64)]) >= 5, "the context is usable afterwards"
