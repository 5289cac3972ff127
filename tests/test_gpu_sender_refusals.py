"""The five packet senders' answers to bad arguments, pinned: status AND full error text of every case of tests/sender_refusal_cases.py,
the last-call records behind every case, and a good call behind every case.  tests/sender_refusals_pinned.json was recorded from the
build before the senders' argument checks, descriptor fill, composed loop and last-call records were folded into one copy each
(python tests/sender_refusal_cases.py --lib OLD.so --out tests/sender_refusals_pinned.json): a check that moved in front of another, a
record written on a refusal or a changed text shows here, where the per-sender tests -- one fault at a time, substrings -- would not."""
import json
import os

import pytest

import sender_refusal_cases as cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PINNED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sender_refusals_pinned.json")


def test_cases_reach_every_entry_point_and_every_precedence_pair():
    names = [c[0] for c in cases.CASES]
    assert len(set(names)) == len(names)
    for kind in cases.KINDS:
        for what in ("good call", "no frames", "unknown handle", "S = 0", "S = 24 at unit 16", "2^31 packets, null pointers", "host source",
                     "host packets", "word-sized S, source at an odd address", "packets begin inside source", "source begins inside packets",
                     "unknown handle + S = 0", "S = 24 + no frames", "2^31 packets + host pointers", "S = 24 + host source", "host pointers + overlap"):
            assert f"{kind}: {what}" in names
    for kind in cases.DEPTH_KINDS:
        assert f"{kind}: depth 3" in names and f"{kind}: depth 3 + no frames" in names
    for kind in cases.LDPC_KINDS:
        assert f"{kind}: non-triangular code" in names and f"{kind}: non-triangular code + S = 24" in names


def test_the_senders_answer_as_pinned():
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
    assert all(r[2] == "same bytes" for r in got if r[0].endswith(" / usable"))
