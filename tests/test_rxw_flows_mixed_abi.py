"""CPU-side checks of the C ABI of the windowed multi-flow receiver's mixed calls (include/ldpc_erasure_amd_rx_window_flows_mixed.h):
the header declares exactly three symbols, the library exports them with the declared argument types, the binding lists exactly
those, the header is self-contained C99, a NULL object is refused before anything touches a device, and the header of the segmented
calls still declares its own eleven symbols and points here."""
import ctypes as C
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_rx_window_flows_mixed.h")
SEGMENTED = os.path.join(ROOT, "include", "ldpc_erasure_amd_rx_window_flows.h")
LDPC_AMD_EINVAL = -1
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64

# the argument lists of the header, as ctypes sees them
SIGNATURES = {
    "ldpc_amd_fec_rxw_flows_push_mixed": [vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, vp],
    "ldpc_amd_fec_rxw_flows_decode_mixed": [vp, i32, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp],
    "ldpc_amd_fec_rxw_flows_unrouted": [vp],
}


def code_of(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def symbols_of(path):
    return sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", code_of(path))))


def test_mixed_symbols_exported_and_bound():
    syms = symbols_of(HEADER)
    assert syms == sorted(SIGNATURES) and sorted(api.EXPORTS_RX_WINDOW_FLOWS_MIXED) == syms and len(syms) == 3
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert list(getattr(L, s).argtypes) == SIGNATURES[s], f"{s}: the ctypes signature in api.load_library"
    assert L.ldpc_amd_fec_rxw_flows_unrouted.restype is i64


def test_mixed_header_declares_the_argument_lists():
    """The number of parameters of every declaration is the number the binding passes; the order is that of the two-buffer object's
    mixed calls (include/ldpc_erasure_amd_flows_mixed.h)."""
    txt = code_of(HEADER)
    old = code_of(os.path.join(ROOT, "include", "ldpc_erasure_amd_flows_mixed.h"))
    for name, args in SIGNATURES.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        params = [a.strip() for a in m.group(1).split(",") if a.strip()]
        assert len(params) == len(args), name
        mo = re.search(r"\b%s\s*\(([^)]*)\)" % name.replace("_rxw_flows_", "_rx_flows_"), old)
        theirs = [re.sub(r"\s+", " ", a.strip()).replace("ldpc_amd_fec_rx_flows", "ldpc_amd_fec_rxw_flows") for a in mo.group(1).split(",")]
        assert [re.sub(r"\s+", " ", p) for p in params] == theirs, name


def test_mixed_header_states_its_contract():
    txt = open(HEADER).read()
    for words in ("last-copy-wins", "offered[f] = |seg_f|", "left[p] = 1", "P == 0 returns 0", "4-byte aligned", "LDPC_AMD_EHIP",
                  "flow_of is read before the call returns", "ldpc_amd_fec_rxw_flows_info", "before any device is touched"):
        assert words in txt, words
    assert "keep `packets` alive" in txt.replace("Keep", "keep")


def test_mixed_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    uses = " || ".join(f"(int)sizeof(&{s}) == 0" for s in symbols_of(HEADER))
    src.write_text('#include "ldpc_erasure_amd_rx_window_flows_mixed.h"\n' f"int main(void) {{ return {uses}; }}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_mixed_null_handles_are_refused_without_a_device():
    L = api.load_library()
    assert L.ldpc_amd_fec_rxw_flows_push_mixed(None, None, None, 0, None, None, None, None, 1, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_push_mixed(None, None, None, 5, None, None, None, None, 1, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_decode_mixed(None, 0, None, None, 0, 10, 1, None, None, None, None, None, None, None, None, 1, None, None,
                                                 None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_flows_unrouted(None) == -1


def test_python_surface():
    for name in ("push_mixed", "decode_mixed", "unrouted", "push_many", "decode_many", "flush_many", "decode_flush_many"):
        assert hasattr(api.FecRxWindowFlows, name)
    assert isinstance(api.FecRxWindowFlows.unrouted, property)
    assert api.FecRxWindowFlows._mixed is api.FecRxFlows._mixed
    import inspect
    for name in ("push_mixed", "decode_mixed"):
        ours, theirs = inspect.signature(getattr(api.FecRxWindowFlows, name)), inspect.signature(getattr(api.FecRxFlows, name))
        assert list(ours.parameters) == list(theirs.parameters) and ours.parameters["want_left"].default is False, name


def test_segmented_header_keeps_its_symbols_and_names_this_one():
    syms = symbols_of(SEGMENTED)
    assert len(syms) == 11 and sorted(api.EXPORTS_RX_WINDOW_FLOWS) == syms
    assert not set(syms) & set(SIGNATURES)
    txt = open(SEGMENTED).read()
    assert "Out of scope of this header" in txt and "push_mixed / decode_mixed" in txt
    assert "ldpc_erasure_amd_rx_window_flows_mixed.h" in txt
    two = symbols_of(os.path.join(ROOT, "include", "ldpc_erasure_amd_flows_mixed.h"))
    assert len(two) == 5 and sorted(api.EXPORTS_FLOWS_MIXED) == two
