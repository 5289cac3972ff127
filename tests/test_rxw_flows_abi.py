"""CPU-side checks of the windowed multi-flow receiver's C ABI (include/ldpc_erasure_amd_rx_window_flows.h): the library exports
every symbol the header declares with the declared argument types, the binding lists exactly those, the header is self-contained
C99, and a NULL object / context is refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_rx_window_flows.h")
LDPC_AMD_EINVAL = -1
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64

# the argument lists of the header, as ctypes sees them (every pointer but those to one int / int64 is a void pointer)
SIGNATURES = {
    "ldpc_amd_fec_rxw_flows_create": [vp, i32, i32, i32, i32, i32, i32, C.POINTER(vp)],
    "ldpc_amd_fec_rxw_flows_destroy": [vp],
    "ldpc_amd_fec_rxw_flows_push_many": [vp, vp, vp, vp, vp, vp, vp, i32, vp],
    "ldpc_amd_fec_rxw_flows_decode_many": [vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp],
    "ldpc_amd_fec_rxw_flows_flush_many": [vp, vp, i32, vp, vp, vp, vp],
    "ldpc_amd_fec_rxw_flows_decode_flush_many": [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
    "ldpc_amd_fec_rxw_flows_pending": [vp, vp, vp],
    "ldpc_amd_fec_rxw_flows_state": [vp, i32, C.POINTER(i32), vp, C.POINTER(i64)],
    "ldpc_amd_fec_rxw_flows_stats": [vp, i32, C.POINTER(i64)],
    "ldpc_amd_fec_rxw_flows_dropped": [vp, i32],
    "ldpc_amd_fec_rxw_flows_info": [vp, C.POINTER(i64)],
}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_symbols():
    return sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", header_text())))


def test_rxw_flows_symbols_exported_and_bound():
    syms = header_symbols()
    assert syms == sorted(SIGNATURES) and sorted(api.EXPORTS_RX_WINDOW_FLOWS) == syms and len(syms) == 11
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert list(getattr(L, s).argtypes) == SIGNATURES[s], f"{s}: the ctypes signature in api.load_library"
    assert L.ldpc_amd_fec_rxw_flows_destroy.restype is None and L.ldpc_amd_fec_rxw_flows_dropped.restype is i64


def test_rxw_flows_header_declares_the_argument_lists():
    """The number of parameters of every declaration is the number the binding passes."""
    txt = header_text()
    for name, args in SIGNATURES.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name


def test_rxw_flows_header_states_its_contract():
    txt = open(HEADER).read()
    assert "push_mixed" in txt and "Out of scope" in txt, "interleaved packets are named as out of scope"
    assert "keep `packets` alive" in txt.replace("Keep", "keep") and "LDPC_AMD_EHIP" in txt and "LDPC_AMD_ENOMEM" in txt
    single = open(os.path.join(ROOT, "include", "ldpc_erasure_amd_rx_window.h")).read()
    assert "ldpc_erasure_amd_rx_window_flows.h" in single, "the single-flow header points here"


def test_rxw_flows_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    uses = " || ".join(f"(int)sizeof(&{s}) == 0" for s in header_symbols())
    src.write_text('#include "ldpc_erasure_amd_rx_window_flows.h"\n' f"int main(void) {{ return {uses}; }}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_rxw_flows_null_handles_are_refused_without_a_device():
    L = api.load_library()
    t = (C.c_int64 * 5)()
    h = C.c_void_p()
    assert L.ldpc_amd_fec_rxw_flows_create(None, 3, 200, 150, 16, 4, 10, C.byref(h)) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_push_many(None, None, None, None, None, None, None, 1, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_decode_many(None, 0, None, None, 10, 1, None, None, None, None, None, None, None, None, 1,
                                                None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_flush_many(None, None, 0, None, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_decode_flush_many(None, 0, None, 0, 10, 1, None, None, None, None, None, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_pending(None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_state(None, 0, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_stats(None, 0, t) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_dropped(None, 0) == -1
    assert L.ldpc_amd_fec_rxw_flows_info(None, None) == LDPC_AMD_EINVAL
    L.ldpc_amd_fec_rxw_flows_destroy(None)


def test_python_surface():
    for name in ("push_many", "decode_many", "flush_many", "decode_flush_many", "pending", "stats", "state", "dropped", "close",
                 "__enter__", "__exit__"):
        assert hasattr(api.FecRxWindowFlows, name)
    assert callable(api.Context.fec_rx_window_flows) and callable(api.Context.fec_rx_window_flows_info)
    assert api.WindowFlowsPending._fields == ("base", "cnt", "blocks")
