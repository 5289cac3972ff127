"""CPU-side checks of the block-interleaved wire's C ABI (include/ldpc_erasure_amd_interleave.h): the library exports every symbol
the header declares, the binding lists exactly those, the header is self-contained C99, the info arrays are filled, and a NULL
context is refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_interleave.h")
LDPC_AMD_EINVAL = -1


def header_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))


def test_interleave_symbols_exported_and_bound():
    syms = header_symbols()
    assert sorted(api.EXPORTS_INTERLEAVE) == syms and len(syms) == 7
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"


def test_interleave_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    body = " || ".join("(int)sizeof(&%s) == 0" % s for s in header_symbols())
    src.write_text('#include "ldpc_erasure_amd_interleave.h"\n'
                   "int main(void) { return %s || !LDPC_AMD_FEC_ILV_DEPTH_OK(LDPC_AMD_FEC_ILV_MAX_DEPTH) || LDPC_AMD_FEC_ILV_DEPTH_OK(3); }\n" % body)
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_interleave_header_states_the_rule_and_its_costs():
    txt = open(HEADER).read()
    assert "Bursty_Error_Channel_Model_Generator.m" in txt
    for phrase in ("g = D - (base mod D)", "RE-ANCHOR", "2 * depth <= window", "Latency", "all-erased", "D (A + 1)"):
        assert phrase in txt, phrase
    assert api.ILV_DEPTHS == (1, 2, 4, 8, 16)
    assert int(re.search(r"#define\s+LDPC_AMD_FEC_ILV_MAX_DEPTH\s+(\d+)", txt).group(1)) == max(api.ILV_DEPTHS)


def test_interleave_null_context_is_einval_without_a_device():
    L = api.load_library()
    info = (C.c_int64 * 4)(7, 7, 7, 7)
    h = C.c_void_p()
    assert L.ldpc_amd_fec_encode_packets_ilv_dev(None, 0, 16, 1, None, 1, 0, 4, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_sender_ilv_info(None, info) == LDPC_AMD_EINVAL and list(info) == [7, 7, 7, 7]
    assert L.ldpc_amd_fec_rxw_dev_create_depth(None, 200, 150, 16, 8, 10, 4, C.byref(h)) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_dev_depth(None) == -1 and L.ldpc_amd_fec_rxw_depth(None) == -1


def test_layout_fills_its_arrays_and_accepts_null():
    L = api.load_library()
    first = (C.c_int64 * 6)(*[-1] * 6)
    stride = (C.c_int32 * 6)(*[-1] * 6)
    assert L.ldpc_amd_fec_tx_ilv_layout(6, 10, 254, 2, first, stride) == 60
    assert list(first) == [0, 1, 20, 21, 40, 41] and list(stride) == [2] * 6
    assert L.ldpc_amd_fec_tx_ilv_layout(6, 10, 255, 2, first, None) == 60 and list(first) == [0, 10, 11, 30, 31, 50]
    assert L.ldpc_amd_fec_tx_ilv_layout(6, 10, 255, 2, None, stride) == 60 and list(stride) == [1, 2, 2, 2, 2, 1]
