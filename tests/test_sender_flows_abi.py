"""CPU-side checks of the multi-flow sender's C ABI (include/ldpc_erasure_amd_sender_flows.h): the library exports every symbol
the header declares, the binding lists exactly those, the header is self-contained C99, and a NULL context is refused before
anything touches a device."""
import ctypes as C
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_sender_flows.h")
LDPC_AMD_EINVAL = -1


def test_sender_flows_symbols_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(api.EXPORTS_SENDER_FLOWS) == syms and len(syms) == 3
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"


def test_sender_flows_header_cites_the_reference_sender_and_channel():
    txt = open(HEADER).read()
    assert "ldpc_erasure_encoder_VITA_in_UDP_out.cl:84-129,168-211" in txt
    assert "Bursty_Error_Channel_Model_Generator.m" in txt


def test_sender_flows_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ldpc_erasure_amd_sender_flows.h"\n'
                   "int main(void) { return (int)sizeof(&ldpc_amd_fec_tx_flows_layout) == 0 || (int)sizeof(&ldpc_amd_fec_encode_packets_flows_dev) == 0\n"
                   "                 || (int)sizeof(&ldpc_amd_fec_sender_flows_info) == 0 || LDPC_AMD_FEC_TX_SEGMENTED == LDPC_AMD_FEC_TX_ROUND_ROBIN; }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_sender_flows_order_constants_match_the_binding():
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+LDPC_AMD_FEC_TX_SEGMENTED\s+(\d+)", txt).group(1)) == api.TX_SEGMENTED == 0
    assert int(re.search(r"#define\s+LDPC_AMD_FEC_TX_ROUND_ROBIN\s+(\d+)", txt).group(1)) == api.TX_ROUND_ROBIN == 1


def test_sender_flows_null_context_is_einval_without_a_device():
    L = api.load_library()
    fb = (C.c_int64 * 2)(0, 1)
    one = (C.c_uint8 * 1)(1)
    assert L.ldpc_amd_fec_encode_packets_flows_dev(None, 0, 16, 1, fb, None, one, one, 0, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_sender_flows_info(None, None) == LDPC_AMD_EINVAL
