"""CPU-side checks of the datagram C ABI (include/ldpc_erasure_amd_datagrams.h): the library exports every symbol the header
declares, the binding lists exactly those, the header is self-contained C99, the constants match the binding, a NULL context is
refused before anything touches a device, and ldpc_amd_fec_dgram_wire_len -- host arithmetic -- agrees with the numpy model
(tools/datagram_frames.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import datagram_frames as dg  # noqa: E402

HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_datagrams.h")
LDPC_AMD_EINVAL = -1


def test_datagram_symbols_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(api.EXPORTS_DATAGRAMS) == syms and len(syms) == 4
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"


def test_datagram_header_cites_the_reference_sender():
    assert "ldpc_erasure_encoder_VITA_in_UDP_out.cl:140-162" in open(HEADER).read()


def test_datagram_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ldpc_erasure_amd_datagrams.h"\n'
                   "int main(void) { return (int)sizeof(&ldpc_amd_fec_dgram_pack_dev) == 0 || (int)sizeof(&ldpc_amd_fec_dgram_unpack_dev) == 0\n"
                   "                 || (int)sizeof(&ldpc_amd_fec_dgram_wire_len) == 0 || (int)sizeof(&ldpc_amd_fec_dgram_info) == 0\n"
                   "                 || LDPC_AMD_DGRAM_DELIVERED == LDPC_AMD_DGRAM_LOST || LDPC_AMD_DGRAM_PREFIX_BYTES != 4; }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_datagram_constants_match_the_binding_and_the_model():
    txt = open(HEADER).read()

    def const(name):
        return int(re.search(r"#define\s+LDPC_AMD_DGRAM_" + name + r"\s+(\d+)", txt).group(1))

    assert const("DELIVERED") == api.DGRAM_DELIVERED == dg.DELIVERED == 0
    assert const("FILLER") == api.DGRAM_FILLER == dg.FILLER == 1
    assert const("LOST") == api.DGRAM_LOST == dg.LOST == 2
    assert const("MALFORMED") == api.DGRAM_MALFORMED == dg.MALFORMED == 3
    assert const("PREFIX_BYTES") == api.DGRAM_PREFIX_BYTES == dg.PREFIX == 4
    assert api.Datagrams._fields == ("bytes", "offset", "state")


def test_datagram_null_context_is_einval_without_a_device():
    L = api.load_library()
    off = (C.c_int64 * 2)(0, 4)
    assert L.ldpc_amd_fec_dgram_pack_dev(None, None, off, 1, 1, 16, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_dgram_unpack_dev(None, None, None, 1, 2, 1, 16, None, 12, None, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_dgram_info(None, None) == LDPC_AMD_EINVAL


def lengths_to_offsets(ln, first=0):
    return np.concatenate([[first], first + np.cumsum(np.asarray(ln, dtype=np.int64))]).astype(np.int64)


@pytest.mark.parametrize("S", [8, 16, 48, 1460])
@pytest.mark.parametrize("N", [0, 1, 6, 7, 8, 38])
def test_wire_len_is_the_models(S, N):
    rng = np.random.default_rng(S + N)
    n, k = 10, 7
    off = lengths_to_offsets(rng.integers(0, S - 3, size=N), first=5)
    got = api.fec_datagram_wire_len(off, n, k, S)
    assert got.dtype == np.int32 and got.shape == (-(-N // k) * n,)
    assert np.array_equal(got, dg.wire_len(off, n, k, S))


def test_wire_len_all_fillers():
    got = api.fec_datagram_wire_len(np.full(10, 3, dtype=np.int64), 5, 4, 16).reshape(3, 5)
    assert (got[:, :4] == 12).all() and (got[:, 4] == 24).all()
    assert np.array_equal(got.reshape(-1), dg.wire_len(np.full(10, 3), 5, 4, 16))


def test_wire_len_refusals():
    L = api.load_library()
    with pytest.raises(api.LdpcAmdError):
        api.fec_datagram_wire_len([0, 8, 4], 5, 4, 16)          # decreasing
    with pytest.raises(api.LdpcAmdError):
        api.fec_datagram_wire_len([-1, 4], 5, 4, 16)            # negative
    with pytest.raises(api.LdpcAmdError):
        api.fec_datagram_wire_len([0, 13], 5, 4, 16)            # S - 3 bytes
    assert api.fec_datagram_wire_len([0, 12], 5, 4, 16).tolist() == [24, 12, 12, 12, 24]   # S - 4 is fine
    with pytest.raises(api.LdpcAmdError):
        api.fec_datagram_wire_len([0, 4], 5, 4, 10)             # S not a multiple of 4
    with pytest.raises(api.LdpcAmdError):
        api.fec_datagram_wire_len([0, 4], 3, 4, 16)             # n < k
    off = (C.c_int64 * 2)(0, 4)
    assert L.ldpc_amd_fec_dgram_wire_len(1, None, 5, 4, 16, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_dgram_wire_len(-1, off, 5, 4, 16, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_dgram_wire_len(1, off, 5, 4, 16, None) == 5      # wire_len may be NULL: the count alone
