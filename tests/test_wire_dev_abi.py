"""CPU-side checks of the device-resident wire path's C ABI (include/ldpc_erasure_amd_wire_dev.h): the library exports every
symbol the header declares, the binding lists exactly those, and the new header is self-contained C."""
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_wire_dev.h")


def test_wire_dev_symbols_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(api.EXPORTS_WIRE_DEV) == syms and len(syms) == 6
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"


def test_wire_dev_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ldpc_erasure_amd_wire_dev.h"\nint main(void) { return (int)sizeof(&ldpc_amd_fec_rx_dev_push_many) == 0; }\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
