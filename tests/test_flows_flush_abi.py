"""CPU-side checks of the batch flush's C ABI (include/ldpc_erasure_amd_flows_flush.h): the library exports every symbol the header
declares, the binding lists exactly those, the header is self-contained C99 and states the contract, a NULL object / context is
refused before anything touches a device, and the Python surface is there."""
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_flows_flush.h")
LDPC_AMD_EINVAL = -1
NAMES = ("ldpc_amd_fec_rx_flows_pending", "ldpc_amd_fec_rx_flows_flush_many", "ldpc_amd_fec_rx_flows_decode_flush_many",
         "ldpc_amd_fec_flows_flush_info")


def test_flush_symbols_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))
    assert syms == sorted(NAMES) and sorted(api.EXPORTS_FLOWS_FLUSH) == syms
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"


def test_flush_header_states_the_contract():
    txt = open(HEADER).read()
    for word in ("Equality with the loop", "dense in list order", "not touched", "ONE launch", "neither synchronise nor read", "given twice",
                 "rounds outside 1..2", "before any state changes", "EMPTY current block", "256 MiB"):
        assert word in txt, word


def test_flush_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ldpc_erasure_amd_flows_flush.h"\n'
                   "int main(void) { ldpc_amd_fec_rx_flows *rx = 0; (void)rx; return " +
                   " || ".join(f"(int)sizeof(&{n}) == 0" for n in NAMES) + "; }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_flush_null_handles_are_einval_without_a_device():
    L = api.load_library()
    assert L.ldpc_amd_fec_rx_flows_pending(None, None, None, None) == -1
    assert L.ldpc_amd_fec_rx_flows_flush_many(None, None, 0, 2, None, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rx_flows_decode_flush_many(None, 0, None, 0, 2, 10, 1, None, None, None, None, None, None, None,
                                                     None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_flows_flush_info(None, None) == LDPC_AMD_EINVAL


def test_python_surface():
    for name in ("pending", "flush_many", "decode_flush_many"):
        assert callable(getattr(api.FecRxFlows, name))
    assert callable(api.Context.fec_flows_flush_info)
    assert api.FLUSH_PATHS == ("none", "fused", "composed", "push")
