"""GPU tests of the multi-flow receiver's batch flush (include/ldpc_erasure_amd_flows_flush.h): the open blocks of many flows
closed, handed out and decoded by one call.

The expected values are built WITHOUT the code under test: one host reassembler api.FecRx per flow, fed the flow's segments with
the same call boundaries (tools/flow_streams.py, tools/flush_plan.py), gives every flow's drained blocks; the CPU oracle gives the
decoded frames (test_gpu_receiver.oracle_frames); the untouched per-flow loop of decode_flush / flush calls is a second witness.
Slot order comes from the host model tools/flush_plan.py.  What the stream sets hold is asserted without a GPU in
tests/test_flush_plan_cpu.py."""
import os
import sys

import numpy as np
import pytest

from ldpc_erasure_codes_amd import api, codes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_receiver import oracle_frames, random_code, same_frames, to_host  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flow_streams as fs  # noqa: E402
import flush_plan as fp  # noqa: E402

EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


_CODES = {}


def get_code(ctx, which):
    if which not in _CODES:
        if which == "rand":
            code = random_code()
            _CODES[which] = (ctx.register_code(code), code)
        else:
            _CODES[which] = (ctx.load_builtin_code(which, codes.DEFAULT_COEF_SEED[which]), codes.load_builtin(which))
    return _CODES[which]


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def feed(ctx, code, S, sc):
    """A flows object that took every call of the stream set (its closed blocks are not looked at: tests/test_gpu_flows.py does)."""
    rx = ctx.fec_rx_flows(len(sc["flows"]), code.n, code.k, S)
    for call in sc["calls"]:
        pk, fb = fs.call_packets(sc["flows"], call)
        rx.push_many(to_dev(pk), fb, call["mb"])
    return rx


def loop_decode(ctx, rx, h, S, flows, rounds, it=10, do_ml=1):
    """The per-flow loop: (closes, blocks, DecodedFrames on the host) of `rounds` decode_flush calls per listed flow."""
    closes, blocks, frames = [], [], []
    for f in flows:
        c = 0
        for _ in range(rounds):
            r = rx.decode_flush(f, h, max_sweeps=it, do_ml=do_ml)
            if r is None:
                break
            ctx.synchronize()
            blocks.append(r[0])
            frames.append(to_host(r[1], S))
            c += 1
        closes.append(c)
    fr = api.DecodedFrames(*[np.concatenate(x) for x in zip(*frames)]) if frames else None
    return np.array(closes, dtype=np.int32), np.array(blocks, dtype=np.int32), fr


def batch_decode(ctx, rx, h, S, flows, rounds, it=10, do_ml=1):
    closes, blocks, fr = rx.decode_flush_many(h, flows, rounds, max_sweeps=it, do_ml=do_ml)
    ctx.synchronize()
    return closes, blocks, to_host(fr, S) if len(blocks) else None


def host_want(oc, code, S, flushes, it=10, do_ml=1):
    """(blocks, oracle's DecodedFrames) of host flushes [(block, sym, er)] in slot order."""
    if not flushes:
        return np.zeros(0, np.int32), None
    sym = np.stack([s for _, s, _ in flushes]).reshape(-1, code.n, S)
    er = np.stack([e for _, _, e in flushes])
    return np.array([b for b, _, _ in flushes], dtype=np.int32), oracle_frames(oc, code, sym, er, it, do_ml)


def check_drain(ctx, rx, h, oc, code, S, sc, path, it=10, do_ml=1, loop=True):
    """One decode_flush_many(rounds = 2) over all flows of a fed object against the model, the host receivers + oracle and -- loop --
    a second fed object drained by the per-flow loop."""
    nf = len(sc["flows"])
    p = rx.pending()
    model = fp.plan((p.cur_block, p.cur_cnt, p.next_cnt))
    assert p.blocks == len(model["slots"])
    closes, blocks, fr = batch_decode(ctx, rx, h, S, None, 2, it, do_ml)
    info = ctx.fec_flows_flush_info()
    flat = [x for fl in sc["flushes"] for x in fl]
    wb, want = host_want(oc, code, S, flat, it, do_ml)
    assert np.array_equal(closes, [len(fl) for fl in sc["flushes"]]) and np.array_equal(closes, model["closes"])
    assert np.array_equal(blocks, wb) and blocks.tolist() == [b for _, b in model["slots"]]
    same_frames(fr, want, "host receivers + oracle")
    assert info["path"] == path and info["blocks"] == len(wb) and info["launches"] == 1 and info["scratch_bytes"] > 0, info
    assert rx.pending().blocks == 0 and batch_decode(ctx, rx, h, S, None, 2)[1].size == 0
    if loop:
        with feed(ctx, code, S, sc) as rx2:
            lc, lb, lf = loop_decode(ctx, rx2, h, S, range(nf), 2, it, do_ml)
        assert np.array_equal(lc, closes) and np.array_equal(lb, blocks)
        same_frames(fr, lf, "the per-flow loop")
    return want


# ---------------------------------------------------------------------------------------------- 1. equality with the loop
@pytest.mark.parametrize("S", [16, 128])
def test_decode_flush_many_equals_the_loop_host_receivers_and_oracle(ctx, oracle, S):
    h, code = get_code(ctx, "rand")
    oc = oracle.OracleCode(code)
    sc = fp.scenario("mixed", oc, code, S)
    kd = fp.kinds(sc["flushes"], code.k)
    assert kd["two"] and kd["empty_cur"] and kd["nothing"] and kd["short"], kd      # (on the host reference: no vacuous pass)
    with feed(ctx, code, S, sc) as rx:
        want = check_drain(ctx, rx, h, oc, code, S, sc, "fused")
    slot_of = {fj: i for i, fj in enumerate((f, j) for f, fl in enumerate(sc["flushes"]) for j in range(len(fl)))}
    for fj in kd["short"]:                                   # fewer than k symbols: undecodable, and the oracle says how
        assert want.status[slot_of[fj]] in (api.ST_ML_RANKDEF, api.ST_ML_SKIPPED) and want.residual[slot_of[fj]] > 0
    assert want.erased_out[slot_of[(kd["empty_cur"][0], 0)]].all()                  # the empty block comes out all erased


# ---------------------------------------------------------------------------------------------- 2. the push form
@pytest.mark.parametrize("S", [16, 1])
def test_flush_many_equals_the_loop_of_flush_and_the_host_receivers(ctx, oracle, S):
    h, code = get_code(ctx, "rand")
    sc = fp.scenario("mixed", oracle.OracleCode(code), code, S)
    nf = len(sc["flows"])
    flat = [x for fl in sc["flushes"] for x in fl]
    with feed(ctx, code, S, sc) as rx:
        closes, blocks, sym, er = rx.flush_many()
        ctx.synchronize()
        assert ctx.fec_flows_flush_info()["path"] == "push" and ctx.fec_flows_flush_info()["launches"] == 0
        assert rx.pending().blocks == 0
    assert np.array_equal(closes, [len(fl) for fl in sc["flushes"]]) and np.array_equal(blocks, [b for b, _, _ in flat])
    assert np.array_equal(sym.cpu().numpy(), np.stack([s for _, s, _ in flat])) and np.array_equal(er.cpu().numpy(), np.stack([e for _, _, e in flat]))
    with feed(ctx, code, S, sc) as rx2:
        j = 0
        for f in range(nf):
            while True:
                r = rx2.flush(f)
                if r is None:
                    break
                ctx.synchronize()
                assert r[0] == blocks[j] and torch.equal(r[1], sym[j]) and torch.equal(r[2], er[j]), (f, j)
                j += 1
        assert j == len(blocks)


# ---------------------------------------------------------------------------------------------- 3. the composed paths
@pytest.mark.parametrize("case", ["knob", "S1", "words"])
def test_composed_paths_give_the_bytes_of_the_loop(oracle, case):
    S = dict(knob=16, S1=1, words=20)[case]
    with api.Context(0) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        if case == "words":
            c.set_symbol_unit(4)
        if case == "knob":
            c.configure("LDPC_AMD_RX_PKT", 0)
        code = random_code()
        h = c.register_code(code)
        oc = oracle.OracleCode(code)
        sc = fp.scenario("mixed", oc, code, S)
        with feed(c, code, S, sc) as rx:
            check_drain(c, rx, h, oc, code, S, sc, "composed")


# ---------------------------------------------------------------------------------------------- 4. subset, order, rounds
def test_subset_order_rounds_and_the_stream_goes_on(ctx, oracle):
    h, code = get_code(ctx, "rand")
    n, k, S = code.n, code.k, 16
    oc = oracle.OracleCode(code)
    sc = fp.scenario("mixed", oc, code, S)
    nf = len(sc["flows"])
    rxs = fp.host_receivers(sc, n, k, S)
    first = [5, 2, 7]
    with feed(ctx, code, S, sc) as rx:
        p = rx.pending()
        model = fp.plan((p.cur_block, p.cur_cnt, p.next_cnt), first, 1)
        closes, blocks, fr = batch_decode(ctx, rx, h, S, first, 1)
        got1 = [fp.drain(rxs[f], 1) for f in first]
        wb, want = host_want(oc, code, S, [x for fl in got1 for x in fl])
        assert closes.tolist() == [len(fl) for fl in got1] == [1, 0, 1]       # (flow 2 has nothing open: an entry that closes nothing)
        assert np.array_equal(blocks, wb) and blocks.tolist() == [b for _, b in model["slots"]]
        same_frames(fr, want, "first call")
        q = rx.pending()
        for a, b in zip(q[:3], model["state"]):           # the state after the call: flushed flows moved on, the others did not
            assert np.array_equal(a, b)
        # more packets for ALL flows: every flow's stream goes on with two blocks that continue the numbering it has reached
        b0 = [int(q.cur_block[f]) if q.cur_block[f] >= 0 else 40 + f for f in range(nf)]
        more = [fp.tail_flow(oc, code, S, 9000 + 10 * f, b0[f], (0.1, 0.1, 0.5)) for f in range(nf)]
        pk, fb = fs.flow_begin_of(more)
        dc, db, dsym, der, dused = rx.push_many(to_dev(pk), fb, 4)
        ctx.synchronize()
        host = [rxs[f].push_many(more[f], 4) for f in range(nf)]
        assert np.array_equal(dc, [len(x[0]) for x in host]) and np.array_equal(db, np.concatenate([x[0] for x in host]))
        assert dc.sum() > 0 and np.array_equal(dused, [x[3] for x in host])
        assert np.array_equal(dsym.cpu().numpy(), np.concatenate([x[1] for x in host])) and np.array_equal(der.cpu().numpy(), np.concatenate([x[2] for x in host]))
        # the rest, in another order, both rounds
        order = [f for f in range(nf - 1, -1, -1)]
        closes, blocks, fr = batch_decode(ctx, rx, h, S, order, 2)
        wb, want = host_want(oc, code, S, [x for f in order for x in fp.drain(rxs[f], 2)])
        assert np.array_equal(blocks, wb) and closes.sum() == len(wb) and len(wb) > 0
        same_frames(fr, want, "second call")
    for r in rxs:
        assert r.flush() is None
        r.close()


# ---------------------------------------------------------------------------------------------- 5. the built-in code: tier 2, ML stage, undecodable
def test_builtin_code_tails(ctx, oracle):
    h, code = get_code(ctx, 1)
    S = 1024
    oc = oracle.OracleCode(code)
    sc = fp.scenario("builtin", oc, code, S)
    assert [len(fl) for fl in sc["flushes"]] == [1, 1, 1, 2]
    with feed(ctx, code, S, sc) as rx:
        want = check_drain(ctx, rx, h, oc, code, S, sc, "fused", it=1, loop=False)   # one sweep leaves the lossy tails to the ML stage
        plan, names = ctx.last_plan(), ctx.profile_kernel_names()
    lost = np.array([int(er.sum()) for fl in sc["flushes"] for _, _, er in fl])
    assert lost[0] == 1 and want.status[0] == api.ST_MP_DONE                          # complete
    assert names["apply"].startswith("ldpc_scatter_pktin_kernel<")
    assert plan["two_tiers"] == 1 and lost[1] > plan["tier1_cap"] and names["apply_tier2"].startswith("ldpc_scatter_pktin_big_kernel<")
    assert want.status[1] == api.ST_ML_SOLVED and want.status[2] == api.ST_ML_SOLVED  # the ML stage solves both lossy tails
    assert lost[3] > code.n - code.k and set(want.status[3:].tolist()) <= {api.ST_ML_RANKDEF, api.ST_ML_SKIPPED}   # undecodable


# ---------------------------------------------------------------------------------------------- 6. more flows than a wavefront / a workgroup
@pytest.mark.parametrize("name", ["many", "crowd"])
def test_more_flows_than_a_wavefront_and_than_a_workgroup(ctx, oracle, name):
    h, code = get_code(ctx, "rand")
    oc = oracle.OracleCode(code)
    sc = fp.scenario(name, oc, code, 16)
    assert len(sc["flows"]) == dict(many=130, crowd=300)[name]
    with feed(ctx, code, 16, sc) as rx:
        check_drain(ctx, rx, h, oc, code, 16, sc, "fused", loop=name == "many")


# ---------------------------------------------------------------------------------------------- 7. the planes are reset
@pytest.mark.parametrize("form", ["decode", "push"])
def test_planes_are_reset(ctx, oracle, form):
    h, code = get_code(ctx, "rand")
    n, k, S = code.n, code.k, 16
    oc = oracle.OracleCode(code)
    sc = fp.scenario("mixed", oc, code, S)
    nf = len(sc["flows"])
    with feed(ctx, code, S, sc) as rx:
        if form == "decode":
            rx.decode_flush_many(h)
        else:
            rx.flush_many()
        q = rx.pending()
        assert q.blocks == 0
        # a fresh stream set that goes on where every flow's numbering stands; lossy blocks, so that a stale row would show
        b0 = [int(q.cur_block[f]) if q.cur_block[f] >= 0 else 40 + f for f in range(nf)]
        more = [fp.tail_flow(oc, code, S, 9500 + 10 * f, b0[f], (0.1, 0.15, 0.5)) for f in range(nf)]
        pk, fb = fs.flow_begin_of(more)
        new = [api.FecRx(n, k, S) for _ in range(nf)]
        host = [r.push_many(m, 4) for r, m in zip(new, more)]
        with ctx.fec_rx_flows(nf, n, k, S) as fresh:
            outs = []
            for obj in (rx, fresh):
                dc, db, dsym, der, _ = obj.push_many(to_dev(pk), fb, 4)
                fc, fb2, fsym, fer = obj.flush_many()
                ctx.synchronize()
                outs.append([dc, db, dsym.cpu().numpy(), der.cpu().numpy(), fc, fb2, fsym.cpu().numpy(), fer.cpu().numpy()])
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
        dc, db, dsym, der, fc, fb2, fsym, fer = outs[0]
        assert dc.sum() > 0 and np.array_equal(db, np.concatenate([x[0] for x in host]))
        assert np.array_equal(dsym, np.concatenate([x[1] for x in host])) and np.array_equal(der, np.concatenate([x[2] for x in host]))
        tail = [x for r in new for x in fp.drain(r, 2)]
        assert fb2.tolist() == [b for b, _, _ in tail] and len(tail) > 0
        assert np.array_equal(fsym, np.stack([s for _, s, _ in tail])) and np.array_equal(fer, np.stack([e for _, _, e in tail]))
    for r in new:
        r.close()


# ---------------------------------------------------------------------------------------------- 8. guard bands
@pytest.mark.parametrize("knob", [None, 0])
def test_guard_bands_and_untouched_slots(ctx, oracle, knob):
    h, code = get_code(ctx, "rand")
    n, k, S, G = code.n, code.k, 16, 4096
    sc = fp.scenario("mixed", oracle.OracleCode(code), code, S)
    nf = len(sc["flows"])
    slots = nf * 2
    want_T = sum(len(fl) for fl in sc["flushes"])
    assert 0 < want_T < slots
    L = ctx._L
    sizes = dict(out=slots * n * S, sweeps=4 * slots, residual=4 * slots, status=4 * slots, erased_out=slots * n, residual_src=4 * slots,
                 sym=slots * n * S, er=slots * n)

    def fresh_bufs():
        bufs = {kk: torch.full((v + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda") for kk, v in sizes.items()}
        return bufs, {kk: bufs[kk].data_ptr() + G for kk in bufs}

    def dec(rx, ptr, blocks, closes):
        return L.ldpc_amd_fec_rx_flows_decode_flush_many(rx._h, h, None, 0, 2, 10, 1, ptr["out"], ptr["sweeps"], ptr["residual"], ptr["status"],
                                                         ptr["erased_out"], ptr["residual_src"], blocks[1:].ctypes.data, closes[1:].ctypes.data)

    def push(rx, ptr, blocks, closes):
        return L.ldpc_amd_fec_rx_flows_flush_many(rx._h, None, 0, 2, ptr["sym"], ptr["er"], blocks[1:].ctypes.data, closes[1:].ctypes.data)

    ctx.configure("LDPC_AMD_RX_PKT", knob)
    try:
        for call, mine in ((dec, ("out", "sweeps", "residual", "status", "erased_out", "residual_src")), (push, ("sym", "er"))):
            bufs, ptr = fresh_bufs()
            blocks, closes = np.full(slots + 2, -7, dtype=np.int32), np.full(nf + 2, -7, dtype=np.int32)
            with ctx.fec_rx_flows(nf, n, k, S) as rx0:               # T == 0 on a fresh object: nothing is touched
                assert call(rx0, ptr, blocks, closes) == 0
                ctx.synchronize()
            assert (blocks == -7).all() and (closes[1:1 + nf] == 0).all() and closes[0] == -7 and (closes[1 + nf:] == -7).all()
            for kk in sizes:
                assert bool((bufs[kk] == 0xA5).all()), kk
            closes[:] = -7
            with feed(ctx, code, S, sc) as rx:
                T = call(rx, ptr, blocks, closes)
                ctx.synchronize()
            assert T == want_T and closes[1:1 + nf].tolist() == [len(fl) for fl in sc["flushes"]]
            assert closes[0] == -7 and (closes[1 + nf:] == -7).all() and blocks[0] == -7 and (blocks[1 + T:] == -7).all()
            assert blocks[1:1 + T].tolist() == [b for fl in sc["flushes"] for b, _, _ in fl]
            for kk, v in sizes.items():
                host = bufs[kk].cpu().numpy()
                if kk not in mine:
                    assert (host == 0xA5).all(), kk
                    continue
                per = v // slots
                assert (host[:G] == 0xA5).all() and (host[G + v:] == 0xA5).all(), kk
                assert (host[G + T * per:G + v] == 0xA5).all(), f"{kk}: slots at or beyond the total were touched"
                assert not (host[G:G + T * per] == 0xA5).all(), kk
    finally:
        ctx.configure("LDPC_AMD_RX_PKT", None)


# ---------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_leave_every_flow_where_it_was(ctx, oracle):
    L = ctx._L
    h, code = get_code(ctx, "rand")
    hb, _ = get_code(ctx, 1)
    n, k, S = code.n, code.k, 16
    oc = oracle.OracleCode(code)
    sc = fp.scenario("mixed", oc, code, S)
    nf = len(sc["flows"])
    slots = 2 * nf
    out = torch.full((slots, n, S), 0xA5, dtype=torch.uint8, device="cuda")
    er = torch.full((slots, n), 0xA5, dtype=torch.uint8, device="cuda")
    out_host = np.zeros((slots, n, S), dtype=np.uint8)
    er_host = np.zeros((slots, n), dtype=np.uint8)
    blocks, closes = np.full(slots, -7, dtype=np.int32), np.full(nf, -7, dtype=np.int32)

    def refused(rc, text):
        assert rc == EINVAL, rc
        msg = L.ldpc_amd_last_error(ctx._h)
        assert msg and text in msg, msg

    def ids(*v):
        return np.array(v, dtype=np.int32)

    with feed(ctx, code, S, sc) as rx:
        before = rx.pending()
        info = ctx.fec_flows_flush_info()

        def dec(flows=None, nsel=0, rounds=2, code_h=h, out_p=out.data_ptr(), er_p=er.data_ptr()):
            return L.ldpc_amd_fec_rx_flows_decode_flush_many(rx._h, code_h, flows.ctypes.data if flows is not None else None, nsel, rounds, 10, 1,
                                                             out_p, None, None, None, er_p, None, blocks.ctypes.data, closes.ctypes.data)

        def push(flows=None, nsel=0, rounds=2, out_p=out.data_ptr(), er_p=er.data_ptr(), **kw):
            return L.ldpc_amd_fec_rx_flows_flush_many(rx._h, flows.ctypes.data if flows is not None else None, nsel, rounds, out_p, er_p,
                                                      blocks.ctypes.data, closes.ctypes.data)

        for call in (dec, push):
            refused(call(ids(1, 3, 1), 3), b"given twice")
            refused(call(ids(1, nf), 2), b"no flow")
            refused(call(ids(-1), 1), b"no flow")
            refused(call(ids(*range(nf), 0), nf + 1), b"nsel")
            refused(call(ids(0), -1), b"nsel")
            refused(call(rounds=0), b"rounds must be 1 or 2")
            refused(call(rounds=3), b"rounds must be 1 or 2")
            refused(call(out_p=out_host.ctypes.data), b"device pointers")
            refused(call(er_p=er_host.ctypes.data), b"device pointers")
        refused(dec(code_h=hb), b"(2040,1530)")
        assert L.ldpc_amd_fec_rx_flows_decode_flush_many(rx._h, 999, None, 0, 2, 10, 1, out.data_ptr(), None, None, None, None, None, None,
                                                         None) == -4                                          # LDPC_AMD_ENOCODE
        refused(L.ldpc_amd_fec_rx_flows_decode_flush_many(rx._h, h, None, 0, 2, 0, 1, out.data_ptr(), None, None, None, None, None, None, None),
                b"max_sweeps")
        # nsel == 0 with a list: returns 0, nothing is touched
        assert dec(ids(0), 0) == 0 and push(ids(0), 0) == 0
        ctx.synchronize()
        after = rx.pending()
        assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before.blocks == after.blocks
        assert bool((out == 0xA5).all()) and bool((er == 0xA5).all()) and (blocks == -7).all() and (closes == -7).all()
        assert ctx.fec_flows_flush_info() == info
        check_drain(ctx, rx, h, oc, code, S, sc, "fused", loop=False)   # the drain behind the refusals returns the reference's values
