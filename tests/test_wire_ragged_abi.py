"""CPU-side checks of the trimmed-wire C ABI (include/ldpc_erasure_amd_wire_ragged.h): the library exports every symbol the header
declares, the binding lists exactly those, the header is self-contained C99, the constants match the binding and the numpy model
(tools/wire_ragged.py), and a NULL context is refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess
import sys

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wire_ragged as wr  # noqa: E402

HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_wire_ragged.h")
LDPC_AMD_EINVAL = -1


def test_wire_ragged_symbols_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(api.EXPORTS_WIRE_RAGGED) == syms and len(syms) == 3
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"


def test_wire_ragged_header_says_what_trim_does_not_check_and_what_land_may_touch():
    txt = " ".join(re.sub(r"(?m)^ \*", "", open(HEADER).read()).split())   # (the comment's text without its line breaks)
    assert "NOT CHECKED: that the bytes cut off are zero" in txt
    assert "up to 3 bytes that share an aligned dword" in txt
    assert "ldpc_erasure_encoder_VITA_in_UDP_out.cl:140-162" in txt


def test_wire_ragged_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ldpc_erasure_amd_wire_ragged.h"\n'
                   "int main(void) { return (int)sizeof(&ldpc_amd_fec_wire_trim_dev) == 0 || (int)sizeof(&ldpc_amd_fec_wire_land_dev) == 0\n"
                   "                 || (int)sizeof(&ldpc_amd_fec_wire_ragged_info) == 0 || LDPC_AMD_WIRE_LANDED == LDPC_AMD_WIRE_REJECTED; }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_wire_ragged_constants_match_the_binding_and_the_model():
    txt = open(HEADER).read()

    def const(name):
        return int(re.search(r"#define\s+LDPC_AMD_WIRE_" + name + r"\s+(\d+)", txt).group(1))

    assert const("LANDED") == api.WIRE_LANDED == wr.LANDED == 0
    assert const("REJECTED") == api.WIRE_REJECTED == wr.REJECTED == 1
    assert wr.FEC_HEADER == 8 and wr.PREFIX == api.DGRAM_PREFIX_BYTES
    assert api.Wire._fields == ("bytes", "offset")


def test_wire_ragged_null_context_is_einval_without_a_device():
    L = api.load_library()
    info = (C.c_int64 * 3)()
    assert L.ldpc_amd_fec_wire_trim_dev(None, None, 1, 1, 16, None, 24, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_wire_land_dev(None, None, 0, None, 1, 16, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_wire_ragged_info(None, info) == LDPC_AMD_EINVAL
