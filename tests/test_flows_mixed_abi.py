"""CPU-side checks of the mixed calls' C ABI (include/ldpc_erasure_amd_flows_mixed.h): the library exports every symbol the header
declares, the binding lists exactly those, the header is self-contained C99 and states the contract and the scratch bound, a NULL
object / context is refused before anything touches a device, and the Python surface is there."""
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_flows_mixed.h")
LDPC_AMD_EINVAL = -1


def test_mixed_symbols_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(api.EXPORTS_FLOWS_MIXED) == syms and len(syms) == 5
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"
    assert L.ldpc_amd_fec_rx_flows_unrouted.restype is api.C.c_int64 and L.ldpc_amd_fec_flows_demux_dev.restype is api.C.c_int64


def test_mixed_header_states_the_contract():
    txt = open(HEADER).read()
    assert "ldpc_erasure_decoder_with_reordering_logic.cl:44-141,214-243" in txt
    for word in ("keep `packets` alive", "last-copy-wins", "unrouted", "4-byte aligned", "2^31", "in any order", "capped at 1024",
                 "16 MiB + 64 KiB", "before any state changes"):
        assert word in txt, word


def test_mixed_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    names = ("rx_flows_push_mixed", "rx_flows_decode_mixed", "rx_flows_unrouted", "flows_demux_dev", "flows_demux_info")
    src.write_text('#include "ldpc_erasure_amd_flows_mixed.h"\n'
                   "int main(void) { ldpc_amd_fec_rx_flows *rx = 0; (void)rx; return " +
                   " || ".join(f"(int)sizeof(&ldpc_amd_fec_{n}) == 0" for n in names) + "; }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_mixed_null_handles_are_einval_without_a_device():
    L = api.load_library()
    assert L.ldpc_amd_fec_rx_flows_push_mixed(None, None, None, 0, None, None, None, None, 1, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rx_flows_decode_mixed(None, 0, None, None, 0, 10, 1, None, None, None, None, None, None, None, None, 1, None, None,
                                                None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rx_flows_unrouted(None) == -1
    assert L.ldpc_amd_fec_flows_demux_dev(None, None, 0, 1, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_flows_demux_info(None, None) == LDPC_AMD_EINVAL


def test_python_surface():
    for name in ("push_mixed", "decode_mixed"):
        assert callable(getattr(api.FecRxFlows, name))
    assert isinstance(api.FecRxFlows.unrouted, property)
    assert callable(api.Context.fec_flows_demux) and callable(api.Context.fec_flows_demux_info)
