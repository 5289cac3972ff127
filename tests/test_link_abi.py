"""CPU-side checks of the link emulator's C ABI (include/ldpc_erasure_amd_link.h): the library exports every symbol the header
declares, the binding lists exactly those, the header is self-contained C99, the constants match the binding and the numpy model
(tools/link_model.py), a NULL context is refused before anything touches a device, and the header states the two rules a caller
must know."""
import ctypes as C
import os
import re
import subprocess

import link_cases as cases
from ldpc_erasure_codes_amd import api
from link_cases import lm

ROOT = cases.ROOT
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_link.h")
LDPC_AMD_EINVAL = -1


def test_link_symbols_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ldpc_amd_fec_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(api.EXPORTS_LINK) == syms and len(syms) == 4
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"
    assert hasattr(api.Context, "fec_link") and hasattr(api.Context, "fec_link_info")
    assert all(hasattr(api.FecLink, m) for m in ("plan", "send", "send_wire", "first"))


def test_link_header_compiles_as_c99_and_the_struct_is_the_bindings(tmp_path):
    src = tmp_path / "t.c"
    fields = ["seed", "first", "window", "flags", "dup", "bad_sym", "foreign"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ldpc_erasure_amd_link.h"\n'
                   "int main(void) {\n"
                   "    if (sizeof(&ldpc_amd_fec_link_plan_dev) == 0 || sizeof(&ldpc_amd_fec_link_apply_dev) == 0 ||\n"
                   "        sizeof(&ldpc_amd_fec_link_apply_ragged_dev) == 0 || sizeof(&ldpc_amd_fec_link_info) == 0) return 1;\n"
                   '    printf("%d", (int)sizeof(ldpc_amd_link_params));\n'
                   + "".join(f'    printf(" %d", (int)offsetof(ldpc_amd_link_params, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = tmp_path / "t"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(api.LinkParams) == 48
    assert got[1:] == [getattr(api.LinkParams, f).offset for f in fields]
    assert [f for f, _ in api.LinkParams._fields_] == fields == list(lm.Params._fields)


def test_link_constants_match_the_binding_and_the_model():
    txt = open(HEADER).read()

    def const(name):
        return int(re.search(r"#define\s+LDPC_AMD_LINK_" + name + r"\s+(\d+)u?\b", txt).group(1))

    assert const("STREAM_DUP") == api.LINK_STREAM_DUP == lm.STREAM_DUP == 16
    assert const("STREAM_DELAY") == api.LINK_STREAM_DELAY == lm.STREAM_DELAY == 17
    assert const("STREAM_DAMAGE") == api.LINK_STREAM_DAMAGE == lm.STREAM_DAMAGE == 18
    assert const("MAX_WINDOW") == api.LINK_MAX_WINDOW == lm.MAX_WINDOW == 4096 == max(cases.WS)
    assert const("DUP_FLIP") == api.LINK_DUP_FLIP == lm.DUP_FLIP == 1
    assert const("COPY") == api.LINK_COPY == lm.COPY == 1
    assert const("BADSYM") == api.LINK_BADSYM == lm.BADSYM == 2
    assert const("FOREIGN") == api.LINK_FOREIGN == lm.FOREIGN == 4
    assert const("FLIPPED") == api.LINK_FLIPPED == lm.FLIPPED == 8
    # the new stream ids collide with none of the generator's
    synth_h = open(os.path.join(ROOT, "include", "ldpc_erasure_amd_synth.h")).read()
    taken = {int(v) for v in re.findall(r"#define\s+LDPC_SYNTH_STREAM_\w+\s+(\d+)u", synth_h)}
    assert len(taken) == 6 and not taken & {16, 17, 18}
    assert lm.TILE == cases.TILE == 256 and lm.FEC_HEADER == 8


def test_link_null_context_is_einval_without_a_device():
    L = api.load_library()
    info = (C.c_int64 * 4)()
    pr = api.LinkParams(1, 0, 0, 0, 0.0, 0.0, 0.0)
    assert L.ldpc_amd_fec_link_plan_dev(None, C.byref(pr), 1, None, None, None, 2, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_link_apply_dev(None, None, 1, 16, None, None, None, 2, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_link_apply_ragged_dev(None, None, 0, None, 1, None, None, None, 2, None, 0, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_link_info(None, info) == LDPC_AMD_EINVAL


def test_link_header_states_the_call_boundary_and_the_capacity_rule():
    txt = " ".join(re.sub(r"(?m)^ \*", "", open(HEADER).read()).split())   # (the comment's text without its line breaks)
    assert "PACKETS DO NOT CROSS A CALL BOUNDARY" in txt
    assert "two calls of P1 and P2 packets make the draws of one call of P1 + P2 packets" in txt
    assert "must be at least 2 * npackets (cap >= 2P)" in txt
    assert "bytes_cap, the size of bytes_out, must be at least 2 * nbytes" in txt
    assert "Milcom_2022_ErasureCodes.tex:230" in txt
