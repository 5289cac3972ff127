"""CPU-side checks of the C ABI of include/ldpc_erasure_amd_rx_rule.h (the close rule of the windowed receivers as a value): the
library exports every symbol the header declares with the declared argument types, the binding lists exactly those, the header is
self-contained C99, the presets give the documented numbers, invalid rules are refused field by field, get_rule returns what create
was given, and null arguments are refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_rx_rule.h")
LDPC_AMD_EINVAL = -1
vp, i32, rp = C.c_void_p, C.c_int32, C.POINTER(api.RxRule)

# the argument lists of the header, as ctypes sees them
SIGNATURES = {
    "ldpc_amd_fec_rx_rule_default": [i32, i32, rp],
    "ldpc_amd_fec_rx_rule_mds": [i32, i32, i32, i32, rp],
    "ldpc_amd_fec_rx_rule_check": [i32, rp],
    "ldpc_amd_fec_rxw_create_rule": [i32, i32, i32, i32, i32, i32, rp, C.POINTER(vp)],
    "ldpc_amd_fec_rxw_dev_create_rule": [vp, i32, i32, i32, i32, i32, i32, rp, C.POINTER(vp)],
    "ldpc_amd_fec_rxw_flows_create_rule": [vp, i32, i32, i32, i32, i32, i32, i32, rp, C.POINTER(vp)],
    "ldpc_amd_fec_rxw_get_rule": [vp, rp],
    "ldpc_amd_fec_rxw_dev_get_rule": [vp, rp],
    "ldpc_amd_fec_rxw_flows_get_rule": [vp, rp],
}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_symbols():
    return sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", header_text())))


def test_symbols_exported_and_bound():
    syms = header_symbols()
    assert syms == sorted(SIGNATURES) and sorted(api.EXPORTS_RX_RULE) == syms and len(syms) == 9
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert list(getattr(L, s).argtypes) == SIGNATURES[s], f"{s}: the ctypes signature in api.load_library"
    assert C.sizeof(api.RxRule) == 16 and [f[0] for f in api.RxRule._fields_] == ["c_hi", "later_hi", "c_lo", "later_lo"]


def test_header_declares_the_argument_lists():
    """The number of parameters of every declaration is the number the binding passes; the struct has the four fields in order."""
    txt = header_text()
    for name, args in SIGNATURES.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
    assert re.search(r"typedef struct\s*\{\s*int32_t c_hi, later_hi, c_lo, later_lo;\s*\}\s*ldpc_amd_fec_rx_rule;", txt)


def test_header_states_its_contract():
    txt = open(HEADER).read()
    for phrase in ("c >= c_hi && later >= later_hi", "c >= c_lo && later >= later_lo", "(kd + 1, 11, km + 1, 101)", "(k, 1, 0, giveup)",
                   "max(1, depth * k / 2)", "ROUGHLY IN ORDER", "ANY k", "give-up clause", "A + 1", "VALID RULES", "later_* >= 1",
                   "re-anchor", "erased if it is empty", "A NULL rule means"):
        assert phrase in txt, phrase
    rs = open(os.path.join(ROOT, "include", "ldpc_erasure_amd_rs_wire.h")).read()
    assert "THE CLOSE RULE ON SHORT BLOCKS" in rs and "ldpc_erasure_amd_rx_rule.h" in rs, "the RS header points to the rule"


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    uses = " || ".join(f"(int)sizeof(&{s}) == 0" for s in header_symbols())
    src.write_text('#include "ldpc_erasure_amd_rx_rule.h"\n'
                   f"int main(void) {{ ldpc_amd_fec_rx_rule r = {{1, 2, 3, 4}}; return r.c_hi == 0 || {uses}; }}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def as_tuple(r):
    return (r.c_hi, r.later_hi, r.c_lo, r.later_lo)


@pytest.mark.parametrize("n,k,default", [(2040, 1530, (1939, 11, 1633, 101)), (255, 192, (243, 11, 206, 101)), (200, 150, (191, 11, 161, 101))])
def test_presets(n, k, default):
    """kd = k + round(0.8 (n-k)), km = k + round(0.2 (n-k)): 1938 / 1632, 242 / 205, 190 / 160."""
    L = api.load_library()
    r = api.RxRule()
    assert L.ldpc_amd_fec_rx_rule_default(n, k, C.byref(r)) == 0 and as_tuple(r) == default == api.fec_rx_rule_default(n, k)
    assert L.ldpc_amd_fec_rx_rule_check(n, C.byref(r)) == 0
    for depth in (1, 2, 4, 8, 16):
        assert L.ldpc_amd_fec_rx_rule_mds(n, k, depth, 0, C.byref(r)) == 0
        assert as_tuple(r) == (k, 1, 0, max(1, depth * k // 2)) == api.fec_rx_rule_mds(n, k, depth)
        assert L.ldpc_amd_fec_rx_rule_check(n, C.byref(r)) == 0
    assert api.fec_rx_rule_mds(n, k, 8, 777) == (k, 1, 0, 777)
    assert api.fec_rx_rule_mds(n, k) == (k, 1, 0, k // 2)
    for bad in [(n, k, 3, 0), (n, k, 0, 0), (n, k, 32, 0), (n, k, 1, -1), (n, k, 1, (1 << 30) + 1), (n, n, 1, 0), (n, 0, 1, 0), (0, 0, 1, 0)]:
        assert L.ldpc_amd_fec_rx_rule_mds(*bad, C.byref(r)) == -1, bad
    assert L.ldpc_amd_fec_rx_rule_default(n, n, C.byref(r)) == -1 and L.ldpc_amd_fec_rx_rule_default(0, 0, C.byref(r)) == -1
    with pytest.raises(api.LdpcAmdError):
        api.fec_rx_rule_mds(n, k, depth=3)


def test_default_rule_is_valid_for_every_code():
    """n - k <= 2 makes kd = n: c_hi stays at n (c >= n adds nothing to c == n), so no code is left without a valid default rule."""
    L = api.load_library()
    r = api.RxRule()
    for n, k in [(2, 1), (3, 1), (3, 2), (10, 9), (10, 8), (65536, 65535), (65536, 1)]:
        assert L.ldpc_amd_fec_rx_rule_default(n, k, C.byref(r)) == 0 and L.ldpc_amd_fec_rx_rule_check(n, C.byref(r)) == 0, (n, k)
        assert r.c_hi <= n and r.c_lo <= n
        h = vp()
        assert L.ldpc_amd_fec_rxw_create_rule(n, k, 1, 2, 0, 1, None, C.byref(h)) == 0 and h.value
        L.ldpc_amd_fec_rxw_destroy(h)


N, K = 200, 150
GOOD = [(191, 11, 161, 101), (K, 1, 0, 75), (K, 0, K, 0), (0, 1, 0, 1), (0, 5, 0, 5), (N, 1 << 30, N, 1 << 30), (N, 0, 1, 0), (0, 1, N, 0)]
BAD = [(-1, 11, 161, 101), (191, -1, 161, 101), (191, 11, -1, 101), (191, 11, 161, -1),             # negative values
       (N + 1, 11, 161, 101), (191, 11, N + 1, 101),                                               # c > n
       (191, (1 << 30) + 1, 161, 101), (191, 11, 161, (1 << 30) + 1),                              # later > 2^30
       (0, 0, 161, 101), (191, 11, 0, 0), (0, 0, 0, 0)]                                            # c == 0 with later == 0


def test_check_and_host_creator_refuse_each_invalid_field():
    L = api.load_library()
    for rule in GOOD:
        r = api.RxRule(*rule)
        assert L.ldpc_amd_fec_rx_rule_check(N, C.byref(r)) == 0, rule
        with api.FecRxWindowHost(N, K, 16, 4, 10, rule=rule) as rx:
            assert rx.rule == rule
    for rule in BAD:
        r = api.RxRule(*rule)
        assert L.ldpc_amd_fec_rx_rule_check(N, C.byref(r)) == -1, rule
        h = vp()
        assert L.ldpc_amd_fec_rxw_create_rule(N, K, 16, 4, 10, 1, C.byref(r), C.byref(h)) == -1 and not h.value, rule
        with pytest.raises(api.LdpcAmdError):
            api.FecRxWindowHost(N, K, 16, 4, 10, rule=rule)
    r = api.RxRule(N, 1, N, 1)
    assert L.ldpc_amd_fec_rx_rule_check(N - 1, C.byref(r)) == -1 and L.ldpc_amd_fec_rx_rule_check(N, C.byref(r)) == 0, "c is checked against n"


def test_get_rule_round_trips_and_creators_agree():
    L = api.load_library()
    for depth, W in [(1, 4), (4, 8)]:
        with api.FecRxWindowHost(N, K, 16, W, 10, depth=depth) as rx:
            assert rx.rule == (191, 11, 161, 101) and rx.depth == depth
        for rule in GOOD:
            with api.FecRxWindowHost(N, K, 16, W, 10, depth=depth, rule=rule) as rx:
                assert rx.rule == rule and rx.depth == depth and rx.state() == {"base": -1, "cnt": [0] * W, "ahead": 0}
    # the refusals of the other create calls still hold with a rule
    h, r = vp(), api.RxRule(K, 1, 0, 75)
    for args in [(N, K, 16, 1, 10, 1), (N, K, 16, 33, 10, 1), (N, K, 16, 4, -1, 1), (N, K, 16, 4, 10, 3), (N, K, 16, 4, 10, 4), (N, N, 16, 4, 10, 1),
                 (N, K, 0, 4, 10, 1)]:
        assert L.ldpc_amd_fec_rxw_create_rule(*args, C.byref(r), C.byref(h)) == -1 and not h.value, args


def test_null_arguments():
    L = api.load_library()
    r = api.RxRule(7, 7, 7, 7)
    h = vp()
    assert L.ldpc_amd_fec_rx_rule_default(N, K, None) == -1 and L.ldpc_amd_fec_rx_rule_mds(N, K, 1, 0, None) == -1
    assert L.ldpc_amd_fec_rx_rule_check(N, None) == -1
    assert L.ldpc_amd_fec_rxw_create_rule(N, K, 16, 4, 10, 1, C.byref(r), None) == -1
    assert L.ldpc_amd_fec_rxw_get_rule(None, C.byref(r)) == -1 and as_tuple(r) == (7, 7, 7, 7)
    assert L.ldpc_amd_fec_rxw_dev_get_rule(None, C.byref(r)) == LDPC_AMD_EINVAL and L.ldpc_amd_fec_rxw_flows_get_rule(None, C.byref(r)) == LDPC_AMD_EINVAL
    assert as_tuple(r) == (7, 7, 7, 7)
    assert L.ldpc_amd_fec_rxw_dev_create_rule(None, N, K, 16, 4, 10, 1, C.byref(r), C.byref(h)) == LDPC_AMD_EINVAL and not h.value
    assert L.ldpc_amd_fec_rxw_flows_create_rule(None, 3, N, K, 16, 4, 10, 1, C.byref(r), C.byref(h)) == LDPC_AMD_EINVAL and not h.value
    assert L.ldpc_amd_fec_rxw_create_rule(N, K, 16, 4, 10, 1, None, C.byref(h)) == 0 and h.value, "a NULL rule is the default rule"
    assert L.ldpc_amd_fec_rxw_get_rule(h, None) == -1
    assert L.ldpc_amd_fec_rxw_get_rule(h, C.byref(r)) == 0 and as_tuple(r) == (191, 11, 161, 101)
    L.ldpc_amd_fec_rxw_destroy(h)


def test_python_surface():
    import inspect
    assert callable(api.fec_rx_rule_default) and callable(api.fec_rx_rule_mds)
    assert inspect.signature(api.fec_rx_rule_mds).parameters["depth"].default == 1 and inspect.signature(api.fec_rx_rule_mds).parameters["giveup"].default == 0
    for cls in (api.FecRxWindowHost, api.FecRxWindow, api.FecRxWindowFlows):
        assert isinstance(cls.rule, property), cls
        assert inspect.signature(cls.__init__).parameters["rule"].default is None, cls
    for fn in (api.Context.fec_rx_window, api.Context.fec_rx_window_flows):
        assert inspect.signature(fn).parameters["rule"].default is None, fn
    with pytest.raises(api.LdpcAmdError):
        api.FecRxWindowHost(N, K, 16, 4, 10, rule=(1, 2, 3))
