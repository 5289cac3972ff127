"""The launch plans of the host side, pinned: which kernel instantiation every entry point picks, with which plan, per knob.

The host half of csrc/kernels.hip decides, per call, the peel shape, the packet kernel's pieces and tiers, the ML stage's kernels and
the encoder's schedule.  tests/launch_plans_pinned.json holds what it decided for the cases below -- last_plan(), the instantiation
names of profile_kernel_names(), whether the last encode ran the grouped schedule, and the path of the fused sender and receiver --
RECORDED ONCE from the library before the host half was restructured (the file's "recorded_from" names the commit).  A change of the
host code that is meant to leave the launches alone must leave every entry equal; the file is never regenerated from such a change.

Every case runs in a fresh Context (neither the kernel names nor the fast path's adaptive skip carry over from another case); its
inputs -- codewords with a few erased symbols per frame -- come from a second context, so the case's context has run nothing else.

    python tests/test_gpu_launch_plans.py --record [FILE] [--commit NAME]     writes the JSON (default: next to this file)"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from ldpc_erasure_codes_amd import api, codes  # noqa: E402

pytestmark = pytest.mark.gpu
PINNED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_plans_pinned.json")
CUS = 256            # compute units of the MI355X: the "deep batch" rules count rounds of frames_per_cu x CUs frames
F = 8                # frames per call where a case does not say otherwise

# (tests/test_gpu_plan_edges.py: BATCHES and VARIANTS -- kept equal to that file's by test_cases_follow_plan_edges below)
PAIRS = [(1, 256), (1, 16), (3, 128), (2, 64)]
EDGE_VARIANTS = [("SCATTER_B", "128"), ("SCATTER_B", "64"), ("SCATTER_TIERS", "1"), ("SCATTER_PAIRS", "0"), ("SCATTER_XL", "0"),
                 ("SCATTER_LISTS", "1"), ("SCATTER_DYN", "0"), ("SCATTER_DYN", "2"), ("SCATTER_DYN", "3"), ("SCATTER_DYN", "4"),
                 ("SCATTER_NT", "0"), ("SCATTER_T2B", "128"), ("PEEL_RELAX", "0"), ("APPLY", "gather")]
S1_KNOBS = [None, ("PEEL_GT", "0"), ("PEEL_GT", "1"), ("PEEL_RELAX", "0"), ("PEEL_WPB", "4")]


def _case(kind, code, S, knob=None, **kw):
    name = f"{kind} code{code} S{S}"
    for key in sorted(kw):
        name += f" {key}={kw[key]}"
    if knob:
        name += f" {knob[0]}={knob[1]}"
    return dict(name=name, kind=kind, code=code, S=S, knob=knob, **kw)


def _cases():
    c = []
    for ci, S in PAIRS + [(1, 1024)]:                      # packet decode, defaults
        for ml in (0, 1):
            c.append(_case("decode", ci, S, do_ml=ml))
    for knob in EDGE_VARIANTS + [("SCATTER_R", "1"), ("SCATTER_R", "4"), ("ML_SOLVE", "0"), ("ML_PI", "0"), ("ML_PI", "2"),
                                 ("ML_OVERLAP", "0"), ("ML_OVERLAP", "1"), ("ML_PACK", "1"), ("ML_SOLVE_B", "64")]:
        c.append(_case("decode", 1, 256, knob))
    for knob in [("SCATTER_R2", "2"), ("SCATTER_R2", "4"), ("SCATTER_T2P", "1"), ("SCATTER_T2P", "4")]:
        c.append(_case("decode", 1, 1024, knob))
    c.append(_case("decode", 1, 256, inplace=1))
    for ci in (1, 3):                                      # S = 1: a short batch and one on the far side of the "deep" rule
        for knob in S1_KNOBS:
            c.append(_case("decode", ci, 1, knob, frames=64))
            c.append(_case("decode", ci, 1, knob, frames="deep"))
    for S in (20, 132):                                    # word form
        c.append(_case("decode", 1, S, unit=4))
        c.append(_case("encode", 1, S, unit=4))
    for ci in (1, 3):                                      # encode
        for S in (1, 256):
            c.append(_case("encode", ci, S))
    for knob in [("ENC_PERSIST", "0"), ("ENC_B", "256"), ("ENC_GROUP", "0"), ("ENC_CLIST", "0"), ("ENC_LIST", "1"), ("APPLY", "gather"),
                 ("SCATTER_R", "4")]:
        c.append(_case("encode", 1, 256, knob))
    c.append(_case("sender", 1, 256))
    c.append(_case("sender", 1, 20, unit=4))
    c.append(_case("sender", 1, 256, ("ENC_PKT", "0")))
    c.append(_case("receiver", 1, 256))
    c.append(_case("receiver", 1, 256, ("RX_PKT", "0")))
    return c


CASES = _cases()
assert len({c["name"] for c in CASES}) == len(CASES)


class Inputs:
    """The second context: codewords per (code, S, frames), built once and left unchanged."""

    def __init__(self):
        import torch
        self.torch = torch
        self.saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("LDPC_AMD_")}
        self.ctx = api.Context(0)
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.ctx.set_symbol_unit(4)
        self.handles, self.made, self.fcu = {}, {}, {}

    def close(self):
        self.ctx.close()
        os.environ.update(self.saved)

    def code(self, ci):
        if ci not in self.handles:
            self.handles[ci] = (codes.load_builtin(ci), self.ctx.load_builtin_code(ci, codes.DEFAULT_COEF_SEED[ci]))
        return self.handles[ci]

    def frames(self, ci, S, nframes):
        """(source, codewords, erased, symbols with the erased ones overwritten) on the device."""
        key = (ci, S, nframes)
        if key not in self.made:
            torch = self.torch
            code, h = self.code(ci)
            g = torch.Generator(device="cuda").manual_seed(100 * ci + S)
            shape = (min(nframes, 64), code.k) + ((S,) if S > 1 else ())
            src = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
            cw = self.ctx.encode(h, src)
            rng = np.random.default_rng(7 * ci + S)
            era = np.zeros((cw.shape[0], code.n), dtype=np.uint8)
            for f in range(cw.shape[0]):
                era[f, rng.choice(code.n, size=3 + f % 5, replace=False)] = 1
            era = torch.from_numpy(era).cuda()
            if nframes > 64:                                # a deep batch: the 64 frames over and over
                reps = (nframes + 63) // 64
                src, cw, era = (t.repeat((reps,) + (1,) * (t.ndim - 1))[:nframes].contiguous() for t in (src, cw, era))
            sym = cw.clone()
            sym[era.bool()] = 0x5A
            self.ctx.synchronize()
            self.made[key] = (src, cw, era, sym)
        return self.made[key]


def run_case(inp, case):
    """One case in a fresh context -> what the host side decided."""
    torch = inp.torch
    ci, S, kind = case["code"], case["S"], case["kind"]
    nframes = case.get("frames", F)
    got = {}
    if nframes == "deep":       # 3 x frames_per_cu x CUs + 1, frames_per_cu from the 64-frame run of the same knobs
        nframes = 3 * inp.fcu[(ci, case["knob"])] * CUS + 1
        got["nframes"] = nframes
    src, cw, era, sym = inp.frames(ci, S, 3 if kind == "receiver" else nframes)
    code = inp.code(ci)[0]
    with api.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        if case.get("unit"):
            ctx.set_symbol_unit(case["unit"])
        h = ctx.load_builtin_code(ci, codes.DEFAULT_COEF_SEED[ci])
        if case["knob"]:
            ctx.configure(*case["knob"])
        if kind == "decode":
            if case.get("inplace"):
                ctx.decode(h, sym.clone(), era, inplace=True)
            else:
                ctx.decode(h, sym, era, do_ml=case.get("do_ml", 1))
        elif kind == "encode":
            ctx.encode(h, src)
        elif kind == "sender":
            ctx.fec_encode_packets_device(h, src)
        else:   # receiver: the packets of three frames, the erased ones lost: the second and third frame close a block each
            pk = inp.ctx.fec_packetize_device(cw, 1, 0)
            pk = pk[~era.reshape(-1).bool()].contiguous()
            with ctx.fec_rx_device(code.n, code.k, S) as rx:
                blocks, _, used = rx.decode_many(h, pk, 8)
                ctx.synchronize()
            got["blocks"] = [int(b) for b in blocks]
        ctx.synchronize()
        got["last_plan"] = ctx.last_plan()
        got["kernels"] = ctx.profile_kernel_names()
        got["last_encode_grouped"] = ctx.encode_info(h)["last_encode_grouped"]
        got["sender_path"] = ctx.fec_sender_info()["path"]
        got["receiver_path"] = ctx.fec_receiver_info()["path"]
    if kind == "decode" and S == 1 and nframes == 64:
        inp.fcu[(ci, case["knob"])] = got["last_plan"]["frames_per_cu"]
    return got


@pytest.fixture(scope="module")
def inputs():
    pytest.importorskip("torch")
    inp = Inputs()
    yield inp
    inp.close()


@pytest.fixture(scope="module")
def pinned():
    with open(PINNED) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_launch_plan(inputs, pinned, case):
    if not codes.have_builtin(case["code"]):
        pytest.skip(f"built-in code {case['code']} is not present")
    if case.get("frames") == "deep" and (case["code"], case["knob"]) not in inputs.fcu:     # (run alone: its 64-frame run first)
        run_case(inputs, next(c for c in CASES if c.get("frames") == 64 and (c["code"], c["knob"]) == (case["code"], case["knob"])))
    want = pinned["cases"][case["name"]]
    got = run_case(inputs, case)
    print(case["name"], json.dumps(got))
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], (case["name"], key, got[key], want[key])


def test_pinned_file_has_no_other_case(pinned):
    assert sorted(pinned["cases"]) == sorted(c["name"] for c in CASES)


def test_cases_follow_plan_edges():
    import test_gpu_plan_edges as edges
    assert [(v[0], v[1]) for v in edges.BATCHES.values()] == PAIRS and edges.VARIANTS == EDGE_VARIANTS


def record(path, commit):
    inp = Inputs()
    try:
        out = {"recorded_from": commit, "cases": {}}
        for case in CASES:
            out["cases"][case["name"]] = run_case(inp, case)
            print(case["name"], json.dumps(out["cases"][case["name"]]), flush=True)
    finally:
        inp.close()
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    assert sys.argv[1] == "--record", __doc__
    rest = sys.argv[2:]
    commit = rest[rest.index("--commit") + 1] if "--commit" in rest else "unknown"
    paths = [a for i, a in enumerate(rest) if a != "--commit" and (i == 0 or rest[i - 1] != "--commit")]
    record(paths[0] if paths else PINNED, commit)
