"""What the streams of tests/test_gpu_flows.py exercise, asserted on the reference side alone (no GPU): every stream goes through
one host api.FecRx per flow with the call boundaries the device object gets (tools/flow_streams.py), and the runs must contain the
situations the multi-flow receiver can get wrong -- staging rows, calls in which one flow closes nothing while another closes a
block, flows that stop at max_blocks_per_flow, block numbers that wrap -- and no block so thin that the draft's close rule stalls.
The channel's and the call boundaries' random draws do not depend on the symbol length, so one S per stream covers them all."""
import os
import sys

import numpy as np
import pytest

from ldpc_erasure_codes_amd import codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import flow_streams as fs  # noqa: E402


def _code(which):
    if which == "rand":
        from test_gpu_receiver import random_code
        return random_code()
    if which == "heavy":
        from test_gpu_sender import heavy_code
        return heavy_code()
    return codes.load_builtin(which)


# (stream, code, S, streams that run in more than one call)
STREAMS = [("mixed", "rand", 16, True), ("heavy", "heavy", 128, True), ("builtin", 1, 128, True), ("many", "rand", 16, False),
           ("words", "rand", 20, True)]


@pytest.fixture(scope="module", params=STREAMS, ids=[s[0] for s in STREAMS])
def stream(request, oracle):
    name, which, S, multi = request.param
    code = _code(which)
    return name, code, S, multi, fs.scenario(name, oracle.OracleCode(code), code, S)


def test_every_block_is_thick_enough_and_closes(stream):
    name, code, S, multi, sc = stream
    closed = fs.closed_per_flow(sc)
    km = fs.min_parity_rx(code.n, code.k)
    for f, F in enumerate(sc["F"]):
        assert sc["received"][f].shape == (F,) and (sc["received"][f] > km).all(), (name, f, sc["received"][f], km)
        if F >= 4:
            assert closed[f] >= F - 3, (name, f, closed[f])
        assert closed[f] <= F + 3
    for f, pk in enumerate(sc["flows"]):     # every packet is consumed, call by call
        assert sum(c["flows"][f]["used"] for c in sc["calls"]) == pk.shape[0]


def test_closed_blocks_hold_staging_rows(stream):
    name, code, S, multi, sc = stream
    if not multi:
        assert len(sc["calls"]) == 1         # one call from the empty state: nothing can be carried
        return
    for f, F in enumerate(sc["F"]):
        if F >= 2:
            assert fs.carried_blocks(sc["flows"][f], sc["calls"], f, code.n) >= 1, (name, f)


def test_mixed_stream_has_the_situations(oracle):
    code = _code("rand")
    sc = fs.scenario("mixed", oracle.OracleCode(code), code, 16)
    closes = np.array([[len(c["blocks"]) for c in call["flows"]] for call in sc["calls"]])
    offered = np.array([[c["c"] for c in call["flows"]] for call in sc["calls"]])
    used = np.array([[c["used"] for c in call["flows"]] for call in sc["calls"]])
    mb = np.array([call["mb"] for call in sc["calls"]])
    # a flow that was given packets closes nothing while another closes a block
    assert (((closes == 0) & (offered > 0)).any(1) & (closes > 0).any(1)).any()
    # a flow stops at max_blocks_per_flow with packets left over while another goes on
    stopped = (closes == mb[:, None]) & (used < offered)
    assert stopped.any() and (stopped.any(1) & ((used == offered) & (offered > 0)).any(1)).any()
    # empty segments beside busy ones, and a call that offers nothing at all is allowed but not needed
    assert ((offered == 0).any(1) & (offered > 0).any(1)).any()
    # block numbers pass 255
    wrapped = [np.concatenate([c["flows"][f]["blocks"] for c in sc["calls"]]) for f in range(len(sc["flows"]))]
    assert any(len(b) > 1 and (np.diff(b.astype(np.int64)) < 0).any() and b.max() == 255 for b in wrapped)
    assert (closes.sum(1) > closes.max(1)).any()          # two flows close blocks in the same call
