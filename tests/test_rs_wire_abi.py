"""CPU-side checks of the C ABI of Reed-Solomon on the FEC wire (include/ldpc_erasure_amd_rs_wire.h): the library exports every symbol
the header declares, the binding lists exactly those, the header is self-contained C and C++, a NULL context or receiver is refused
before anything touches a device, and the layout the sender follows is the interleaver's with n = 255."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import interleave_model as im  # noqa: E402

HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_rs_wire.h")
LDPC_AMD_EINVAL = -1


def header_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))


def test_rs_wire_symbols_exported_and_bound():
    syms = header_symbols()
    assert sorted(api.EXPORTS_RS_WIRE) == syms and len(syms) == 5
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"


def test_rs_wire_header_compiles_as_c_and_as_cpp(tmp_path):
    body = " || ".join("(int)sizeof(&%s) == 0" % s for s in header_symbols())
    text = '#include "ldpc_erasure_amd_rs_wire.h"\nint main(void) { return %s || LDPC_AMD_FEC_CLASS_RS != 2; }\n' % body
    for name, cmd in (("t.c", ["cc", "-std=c99"]), ("t.cpp", ["c++", "-std=c++11"])):
        src = tmp_path / name
        src.write_text(text)
        subprocess.check_call(cmd + ["-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_rs_wire_header_states_the_contract():
    txt = open(HEADER).read()
    for phrase in ("Milcom_2022_ErasureCodes.tex:173", "FECClassCode", "FUSED", "COMPOSED", "ReedSolomonErasureCodes.m:78-81",
                   "THE CLOSE RULE ON SHORT BLOCKS", "LDPC_AMD_ENOCODE", "2^31"):
        assert phrase in txt, phrase
    assert api.FEC_CLASS_RS == int(re.search(r"#define\s+LDPC_AMD_FEC_CLASS_RS\s+(\w+)", txt).group(1), 16) == 2


def test_rs_wire_null_context_is_einval_without_a_device():
    L = api.load_library()
    info = (C.c_int64 * 4)(7, 7, 7, 7)
    used = C.c_int64(5)
    assert L.ldpc_amd_fec_rs_encode_packets_dev(None, 0, 16, 1, None, 2, 0, 8, None) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rs_sender_info(None, info) == LDPC_AMD_EINVAL and list(info) == [7, 7, 7, 7]
    assert L.ldpc_amd_fec_rs_receiver_info(None, info) == LDPC_AMD_EINVAL and list(info) == [7, 7, 7, 7]
    assert L.ldpc_amd_fec_rxw_dev_rs_decode_many(None, 0, None, 0, None, None, None, None, None, 1, C.byref(used)) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_fec_rxw_dev_rs_decode_flush(None, 0, None, None, None, None, None) == LDPC_AMD_EINVAL and used.value == 5


def test_layout_with_n_255_is_the_interleave_models_order():
    n = 255
    for B, block0, D in [(11, 250, 1), (11, 250, 8), (11, 250, 16), (40, 0, 8), (3, 255, 2)]:
        first, stride = api.fec_tx_ilv_layout(B, n, block0, D)
        pos = first[:, None] + np.arange(n, dtype=np.int64)[None, :] * stride[:, None]
        frame, row = im.order(B, n, block0, D)
        assert np.array_equal(np.sort(pos.ravel()), np.arange(B * n))
        assert np.array_equal(frame[pos.ravel()], np.repeat(np.arange(B), n)) and np.array_equal(row[pos.ravel()], np.tile(np.arange(n), B))
