"""The two multi-flow device receivers' answers, pinned: status AND full error text of every case of tests/rx_flows_refusal_cases.py, the
object's whole visible state and the last-call records behind every case, a good call behind every case, and sequences of good calls
through every path of the call skeleton, their outputs as digests.  tests/rx_flows_refusals_pinned.json was recorded from the build
before the two receivers' checks, plan, push, decode, commit, batch flush, create and destroy were folded into one copy each
(python tests/rx_flows_refusal_cases.py --lib OLD.so --out tests/rx_flows_refusals_pinned.json): a check that moved in front of
another, a state or an info word written on a refusal, a changed text or a changed output shows here, where the per-receiver tests --
one fault at a time, substrings -- would not."""
import json
import os

import pytest

import rx_flows_refusal_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PINNED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rx_flows_refusals_pinned.json")


def test_cases_reach_every_entry_point_and_every_precedence_pair():
    names = [c[0] for c in cases.CASES]
    assert len(set(names)) == len(names)
    seg, mixed = ("push_many", "decode_many"), cases.MIXED_CALLS
    push, dec = ("push_many", "push_mixed"), ("decode_many", "decode_mixed")

    def has(calls, *whats, kinds=cases.KINDS):
        for kind in kinds:
            for call in calls:
                for what in whats:
                    assert f"{kind} {call}: {what}" in names, (kind, call, what)

    has(seg, "null flow_begin", "flow_begin[0] != 0", "decreasing flow_begin", "decreasing flow_begin + max_blocks_per_flow = 0")
    has(cases.PACKET_CALLS, "2^31 packets, null pointers", "max_blocks_per_flow = 0", "nflows * max_blocks * n too large", "no packets, null pointers",
        "no packets", "null packets", "host packets", "2^31 packets + max_blocks_per_flow = 0", "max_blocks_per_flow = 0 + no packets")
    has(push, "null sym_batch", "host sym_batch", "host erased_batch", "nflows * max_blocks * n too large + null sym_batch",
        "no packets + host sym_batch", "null sym_batch + host packets")
    has(dec, "null out", "host out", "host result array", "no packets + unknown code handle", "no packets + a code of another (n, k)",
        "no packets + host out", "a code of another (n, k) + max_sweeps = 0", "S = 20 at symbol unit 16 + max_sweeps = 0", "max_sweeps = 0 + host out",
        "host out + host packets")
    has(mixed, "null flow_of", "host flow_of", "misaligned flow_of", "host left", "host packets + misaligned flow_of", "host flow_of + host left",
        "misaligned flow_of + host left")
    has(cases.DECODE_CALLS, "unknown code handle", "a code of another (n, k)", "max_sweeps = 0", "S = 20 at symbol unit 16")
    has(("decode_many",), "unknown code handle + decreasing flow_begin")
    has(("decode_mixed",), "unknown code handle + 2^31 packets")
    has(cases.FLUSH_CALLS, "nsel = -1", "nsel > nflows", "flow -1", "flow nflows", "a flow twice", "an empty object", "nsel > nflows + flow nflows",
        "flow -1 + a flow twice", "a flow twice + flow -1")
    has(cases.FLUSH_CALLS, "rounds = 0", "rounds = 3", "rounds = 0 + a flow twice", kinds=("plain",))
    has(("flush_many",), "null sym_batch", "host erased_batch", "a flow twice + null sym_batch", "null sym_batch + host erased_batch",
        "host sym_batch + an empty object")
    has(("decode_flush_many",), "host out", "a flow twice + unknown code handle", "unknown code handle + max_sweeps = 0", "an empty object + host out")
    has(("create",), "nflows = 0", "nflows = 4097", "k = n", "S = 0", "null out", "null out + nflows = 0")
    has(("create",), "window = 1", "window = 33", "ahead_limit = -1", "depth 3", "2 * depth > window", "an invalid rule", "nflows = 0 + window = 1",
        "window = 1 + depth 3", "depth 3 + an invalid rule", kinds=("win",))
    has(("destroy",), "null object")
    # the good sequences: both objects at S = 16, S = 20 under unit 4, misaligned packets, the composed form; the four scans of the window
    good = [g[0] for g in cases.GOOD]
    for kind in cases.KINDS:
        for what in ("S=16", "S=20 at unit 4", "S=16, packets 4 bytes off", "S=16, rx_pkt = 0"):
            assert f"{kind} {what}" in good
    for what in ("depth 2", "MDS preset", "depth 2, MDS preset"):
        assert f"win S=16, {what}" in good


def test_the_receivers_answer_as_pinned():
    ctx, ctx4 = cases.contexts()
    try:
        got = cases.run(ctx, ctx4)
    finally:
        ctx.close()
        ctx4.close()
    with open(PINNED) as f:
        want = json.load(f)
    assert [r[0] for r in got] == [r[0] for r in want]
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, "\n".join(f"got  {g}\nwant {w}" for g, w in diff[:10])
