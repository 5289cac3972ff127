"""CPU-side checks of the multi-flow receiver's C ABI (include/ldpc_erasure_amd_flows.h): the library exports every symbol the
header declares, the binding lists exactly those, the header is self-contained C99 and states the lifetime rule, a NULL object /
context is refused before anything touches a device, and the Python surface is there."""
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_flows.h")
LDPC_AMD_EINVAL = -1


def test_flows_symbols_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(api.EXPORTS_FLOWS) == syms and len(syms) == 7
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"


def test_flows_header_states_the_contract():
    txt = open(HEADER).read()
    assert "ldpc_erasure_decoder_with_reordering_logic.cl:44-141,214-243" in txt
    assert "keep `packets` alive" in txt
    for word in ("dense in flow order", "max_blocks_per_flow", "2^31 - 2", "LDPC_AMD_ENOMEM", "iteration cap"):
        assert word in txt, word


def test_flows_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    names = ("create", "destroy", "push_many", "decode_many", "flush", "decode_flush", "dropped")
    src.write_text('#include "ldpc_erasure_amd_flows.h"\n'
                   "int main(void) { ldpc_amd_fec_rx_flows *rx = 0; (void)rx; return " +
                   " || ".join(f"(int)sizeof(&ldpc_amd_fec_rx_flows_{n}) == 0" for n in names) + "; }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_flows_null_handles_are_einval_without_a_device():
    L = api.load_library()
    assert L.ldpc_amd_fec_rx_flows_create(None, 4, 300, 200, 16, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rx_flows_push_many(None, None, None, None, None, None, None, 1, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rx_flows_decode_many(None, 0, None, None, 10, 1, None, None, None, None, None, None, None, None, 1,
                                               None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rx_flows_flush(None, 0, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rx_flows_decode_flush(None, 0, 0, 10, 1, None, None, None, None, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rx_flows_dropped(None, 0) == -1
    L.ldpc_amd_fec_rx_flows_destroy(None)


def test_python_surface():
    for name in ("push_many", "decode_many", "flush", "decode_flush", "close", "__enter__", "__exit__"):
        assert callable(getattr(api.FecRxFlows, name))
    assert isinstance(api.FecRxFlows.dropped, property)
    assert callable(api.Context.fec_rx_flows)
