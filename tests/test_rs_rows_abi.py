"""CPU-side checks of the C ABI of the Reed-Solomon decoder on rows in place (include/ldpc_erasure_amd_rs_rows.h, a section of
include/ldpc_erasure_amd_rs_wire.h): the library exports the symbol with the declared signature, the header is self-contained C and
C++ and reaches a caller of the RS wire header, a NULL context is refused before anything touches a device, and the receiver's info
call leaves the caller's words alone on a NULL context."""
import ctypes as C
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_rs_rows.h")
WIRE_HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_rs_wire.h")
LDPC_AMD_EINVAL = -1
# the declaration of the issue, argument by argument
SIGNATURE = ["ldpc_amd_ctx *ctx", "int rs", "int S", "int64_t nblocks", "const uint32_t *src", "const uint8_t *packets", "int64_t npackets",
             "const uint8_t *stage", "int64_t nstage_rows", "uint8_t *msg", "int32_t *received", "int32_t *status", "uint8_t *erased_out"]
CTYPES = {"int": C.c_int, "int64_t": C.c_int64}


def declarations(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return {name: [" ".join(a.split()) for a in args.split(",")] for name, args in re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(([^)]*)\)", txt)}


def test_rs_rows_symbol_exported_with_the_declared_signature():
    decl = declarations(HEADER)
    assert sorted(decl) == sorted(api.EXPORTS_RS_ROWS) == ["ldpc_amd_rs_decode_rows_dev"]
    assert decl["ldpc_amd_rs_decode_rows_dev"] == SIGNATURE
    L = api.load_library()
    fn = L.ldpc_amd_rs_decode_rows_dev
    want = [C.c_void_p if "*" in a else CTYPES[a.split()[0]] for a in SIGNATURE]
    assert fn.argtypes == want and fn.restype is C.c_int


def test_rs_rows_header_compiles_alone_and_through_the_wire_header(tmp_path):
    body = "(int)sizeof(&ldpc_amd_rs_decode_rows_dev) == 0 || LDPC_AMD_ROW_ERASED != 0xFFFFFFFFu || LDPC_AMD_ROW_STAGED != 0x80000000u"
    for header in ("ldpc_erasure_amd_rs_rows.h", "ldpc_erasure_amd_rs_wire.h"):
        text = '#include "%s"\nint main(void) { return %s; }\n' % (header, body)
        for name, cmd in (("t.c", ["cc", "-std=c99"]), ("t.cpp", ["c++", "-std=c++11"])):
            src = tmp_path / name
            src.write_text(text)
            subprocess.check_call(cmd + ["-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    assert (api.ROW_ERASED, api.ROW_STAGED) == (0xFFFFFFFF, 0x80000000)


def test_rs_wire_header_has_the_section_and_the_path_word():
    txt = open(WIRE_HEADER).read()
    for phrase in ("THE DECODER ON ROWS IN PLACE", "ldpc_amd_rs_decode_rows_dev", "never fused", "no composed fallback", "1 fused, 2 composed",
                   "LDPC_AMD_EUNSUP", "nblocks * n >= 2^31"):
        assert phrase in txt, phrase
    assert "path" in api.Context.fec_rs_receiver_info.__doc__ and api.RECEIVER_PATHS == ("none", "fused", "composed")


def test_rs_rows_null_context_is_einval_without_a_device():
    L = api.load_library()
    assert L.ldpc_amd_rs_decode_rows_dev(None, 0, 16, 1, None, None, 0, None, 0, None, None, None, None) == LDPC_AMD_EINVAL
    info = (C.c_int64 * 4)(7, 7, 7, 7)
    assert L.ldpc_amd_fec_rs_receiver_info(None, info) == LDPC_AMD_EINVAL and list(info) == [7, 7, 7, 7]
