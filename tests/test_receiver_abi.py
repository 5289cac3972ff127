"""CPU-side checks of the fused receiver's C ABI (include/ldpc_erasure_amd_receiver.h): the library exports every symbol the
header declares, the binding lists exactly those, the header is self-contained C99, and a NULL receiver / context is refused
before anything touches a device."""
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_receiver.h")
LDPC_AMD_EINVAL = -1


def test_receiver_symbols_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(api.EXPORTS_RECEIVER) == syms and len(syms) == 3
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"
    assert api.RECEIVER_PATHS == ("none", "fused", "composed")


def test_receiver_header_cites_the_reference_receiver_and_the_lifetime_rule():
    txt = open(HEADER).read()
    assert "ldpc_erasure_decoder_with_reordering_logic.cl:44-141,214-243" in txt
    assert "keep `packets` alive" in txt


def test_receiver_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ldpc_erasure_amd_receiver.h"\n'
                   "int main(void) { return (int)sizeof(&ldpc_amd_fec_rx_dev_decode_many) == 0 || (int)sizeof(&ldpc_amd_fec_rx_dev_decode_flush) == 0 ||\n"
                   "                        (int)sizeof(&ldpc_amd_fec_receiver_info) == 0; }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_receiver_null_handles_are_einval_without_a_device():
    L = api.load_library()
    assert L.ldpc_amd_fec_rx_dev_decode_many(None, 0, None, 0, 10, 1, None, None, None, None, None, None, None, 1, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rx_dev_decode_flush(None, 0, 10, 1, None, None, None, None, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_receiver_info(None, None) == LDPC_AMD_EINVAL


def test_python_surface():
    for name in ("decode_many", "decode_flush"):
        assert callable(getattr(api.FecRxDevice, name))
    assert callable(api.Context.fec_receiver_info)
