"""CPU-side checks of the C ABI of include/ldpc_erasure_amd_interleave_flows.h (depth on the multi-flow wire): the library exports
every symbol the header declares with the declared argument types, the binding lists exactly those, the header is self-contained
C99, and a NULL object / context is refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_interleave_flows.h")
LDPC_AMD_EINVAL = -1
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64

# the argument lists of the header, as ctypes sees them
SIGNATURES = {
    "ldpc_amd_fec_tx_flows_ilv_layout": [i32, vp, i32, vp, i32, i32, vp, vp],
    "ldpc_amd_fec_encode_packets_flows_ilv_dev": [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32],
    "ldpc_amd_fec_sender_flows_ilv_info": [vp, C.POINTER(i64)],
    "ldpc_amd_fec_rxw_flows_create_depth": [vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)],
    "ldpc_amd_fec_rxw_flows_depth": [vp],
}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_symbols():
    return sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", header_text())))


def test_symbols_exported_and_bound():
    syms = header_symbols()
    assert syms == sorted(SIGNATURES) and sorted(api.EXPORTS_INTERLEAVE_FLOWS) == syms and len(syms) == 5
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert list(getattr(L, s).argtypes) == SIGNATURES[s], f"{s}: the ctypes signature in api.load_library"
    assert L.ldpc_amd_fec_tx_flows_ilv_layout.restype is i64


def test_header_declares_the_argument_lists():
    """The number of parameters of every declaration is the number the binding passes."""
    txt = header_text()
    for name, args in SIGNATURES.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name


def test_header_states_its_contract():
    txt = open(HEADER).read()
    for phrase in ("WHOLE ALIGNED GROUPS", "block0[f] % D == 0", "c_f % D == 0", "base_r + rank + (j D + i') A_r", "stride * (8 + S)",
                   "ldpc_amd_fec_rxw_create_depth", "rxw_scan_flows_grouped", "Out of scope"):
        assert phrase in txt, phrase
    single = open(os.path.join(ROOT, "include", "ldpc_erasure_amd_interleave.h")).read()
    assert "ldpc_erasure_amd_interleave_flows.h" in single and "Out of scope" not in single, "the single-flow header points here"


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    uses = " || ".join(f"(int)sizeof(&{s}) == 0" for s in header_symbols())
    src.write_text('#include "ldpc_erasure_amd_interleave_flows.h"\n' f"int main(void) {{ return {uses}; }}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_handles_are_refused_without_a_device():
    L = api.load_library()
    info = (C.c_int64 * 4)(7, 7, 7, 7)
    h = C.c_void_p()
    assert L.ldpc_amd_fec_rxw_flows_create_depth(None, 3, 200, 150, 16, 8, 10, 4, C.byref(h)) == LDPC_AMD_EINVAL and not h.value
    assert L.ldpc_amd_fec_rxw_flows_depth(None) == -1
    assert L.ldpc_amd_fec_encode_packets_flows_ilv_dev(None, 0, 16, 1, None, None, None, None, 1, None, None, None, 4) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_sender_flows_ilv_info(None, info) == LDPC_AMD_EINVAL and list(info) == [7, 7, 7, 7]


def test_python_surface():
    import inspect
    assert callable(api.fec_tx_flows_ilv_layout) and callable(api.Context.fec_encode_packets_flows_interleaved_device)
    assert callable(api.Context.fec_sender_flows_ilv_info)
    assert isinstance(api.FecRxWindowFlows.depth, property)
    for fn in (api.Context.fec_rx_window_flows, api.FecRxWindowFlows.__init__, api.Context.fec_tx_flows, api.FecTxFlows.__init__):
        assert inspect.signature(fn).parameters["depth"].default == 1, fn
