"""CPU-side checks of the windowed receiver's C ABI (include/ldpc_erasure_amd_rx_window.h): the library exports every symbol the
header declares, the binding lists exactly those, the header is self-contained C99, the host object refuses bad arguments, and a NULL
receiver / context is refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_rx_window.h")
LDPC_AMD_EINVAL = -1


def header_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))


def test_rx_window_symbols_exported_and_bound():
    syms = header_symbols()
    assert sorted(api.EXPORTS_RX_WINDOW) == syms and len(syms) == 18
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"
    assert api.RX_WINDOW_PATHS == ("none", "fused", "composed")
    assert api.RX_WINDOW_TOTALS == ("bad_symbol", "late", "ahead_total", "resyncs", "closed")


def test_rx_window_header_states_the_rule_and_its_limits():
    txt = open(HEADER).read()
    assert "ldpc_erasure_decoder_with_reordering_logic.cl:139" in txt
    assert "RE-ANCHOR" in txt and "mis-anchors" in txt and "Out of scope" in txt
    assert "keep `packets` alive" in txt
    assert re.search(r"#define LDPC_AMD_RXW_MIN_WINDOW 2\b", txt) and re.search(r"#define LDPC_AMD_RXW_MAX_WINDOW 32\b", txt)
    assert (api.RX_WINDOW_MIN, api.RX_WINDOW_MAX) == (2, 32)
    for i, name in enumerate(("BAD_SYMBOL", "LATE", "AHEAD", "RESYNCS", "CLOSED")):
        assert re.search(rf"#define LDPC_AMD_RXW_{name} {i}\b", txt)


def test_rx_window_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    uses = " || ".join(f"(int)sizeof(&{s}) == 0" for s in header_symbols())
    src.write_text('#include "ldpc_erasure_amd_rx_window.h"\n' f"int main(void) {{ return {uses}; }}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_host_object_argument_refusals():
    L = api.load_library()
    h = C.c_void_p()
    for args in [(0, 1, 16, 4, 10), (200, 0, 16, 4, 10), (200, 200, 16, 4, 10), (200, 150, 0, 4, 10), (65537, 150, 16, 4, 10),
                 (200, 150, 16, 1, 10), (200, 150, 16, 33, 10), (200, 150, 16, 4, -1)]:
        assert L.ldpc_amd_fec_rxw_create(*args, C.byref(h)) == -1, args
    assert L.ldpc_amd_fec_rxw_create(200, 150, 16, 4, 10, None) == -1
    assert L.ldpc_amd_fec_rxw_create(200, 150, 16, 2, 0, C.byref(h)) == 0
    buf = (C.c_uint8 * (200 * 16))()
    used = C.c_long(-5)
    assert L.ldpc_amd_fec_rxw_push(h, None, None, None, None) == -1
    assert L.ldpc_amd_fec_rxw_push_many(h, None, 1, buf, buf, None, 1, C.byref(used)) == -1
    assert L.ldpc_amd_fec_rxw_push_many(h, buf, -1, buf, buf, None, 1, C.byref(used)) == -1
    assert L.ldpc_amd_fec_rxw_push_many(h, buf, 1, buf, buf, None, 0, C.byref(used)) == -1
    assert L.ldpc_amd_fec_rxw_push_many(h, buf, 1, None, buf, None, 1, C.byref(used)) == -1
    assert used.value == -5
    assert L.ldpc_amd_fec_rxw_push_many(h, None, 0, buf, buf, None, 1, C.byref(used)) == 0 and used.value == 0   # npackets = 0
    assert L.ldpc_amd_fec_rxw_stats(h, None) == -1
    assert L.ldpc_amd_fec_rxw_flush(h, None, None, None) == 0 and L.ldpc_amd_fec_rxw_dropped(h) == 0
    L.ldpc_amd_fec_rxw_destroy(h)


def test_rx_window_null_handles_are_refused_without_a_device():
    L = api.load_library()
    t = (C.c_int64 * 5)()
    assert L.ldpc_amd_fec_rxw_push(None, None, None, None, None) == -1
    assert L.ldpc_amd_fec_rxw_push_many(None, None, 0, None, None, None, 1, None) == -1
    assert L.ldpc_amd_fec_rxw_flush(None, None, None, None) == -1
    assert L.ldpc_amd_fec_rxw_stats(None, t) == -1 and L.ldpc_amd_fec_rxw_dropped(None) == -1
    assert L.ldpc_amd_fec_rxw_state(None, None, None, None) == -1
    L.ldpc_amd_fec_rxw_destroy(None)
    h = C.c_void_p()
    assert L.ldpc_amd_fec_rxw_dev_create(None, 200, 150, 16, 4, 10, C.byref(h)) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_dev_push_many(None, None, 0, None, None, None, 1, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_dev_flush(None, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_dev_decode_many(None, 0, None, 0, 10, 1, None, None, None, None, None, None, None, 1, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_dev_decode_flush(None, 0, 10, 1, None, None, None, None, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_dev_stats(None, t) == LDPC_AMD_EINVAL and L.ldpc_amd_fec_rxw_dev_dropped(None) == -1
    assert L.ldpc_amd_fec_rxw_dev_state(None, None, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_info(None, None) == LDPC_AMD_EINVAL
    L.ldpc_amd_fec_rxw_dev_destroy(None)


def test_python_surface():
    for name in ("push_many", "decode_many", "flush", "decode_flush", "stats", "dropped", "close", "state"):
        assert hasattr(api.FecRxWindow, name)
    for name in ("push", "push_many", "flush", "stats", "dropped", "close", "state"):
        assert hasattr(api.FecRxWindowHost, name)
    assert callable(api.Context.fec_rx_window) and callable(api.Context.fec_rx_window_info)
