"""CPU-side checks of the word-sized-symbols C ABI (include/ldpc_erasure_amd_words.h): the header declares the two functions of
the switch, the library exports them, the binding lists exactly those, the header is self-contained C99 and cites the reference's
word-sized payload length, a NULL context is refused before anything touches a device, and Context has both methods."""
import os
import re
import subprocess

from ldpc_erasure_codes_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ldpc_erasure_amd_words.h")
LDPC_AMD_EINVAL = -1


def test_words_symbols_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(ldpc_amd_[a-z0-9_]+)\s*\(", txt)))
    assert syms == ["ldpc_amd_get_symbol_unit", "ldpc_amd_set_symbol_unit"]
    assert sorted(api.EXPORTS_WORDS) == syms
    L = api.load_library()
    for s in syms:
        assert hasattr(L, s), f"{s} declared in the header but not exported"
        assert getattr(L, s).argtypes is not None, f"{s} has no ctypes signature in api.load_library"


def test_words_header_cites_the_reference_and_the_refusal_text():
    txt = open(HEADER).read()
    assert "ldpc_erasure_encoder_VITA_in_UDP_out.cl:141-162" in txt
    assert "S must be 1 or a multiple of 4 that is at least 16 (got %d)" in txt


def test_words_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ldpc_erasure_amd_words.h"\n'
                   "int main(void) { return (int)sizeof(&ldpc_amd_set_symbol_unit) == 0 || (int)sizeof(&ldpc_amd_get_symbol_unit) == 0; }\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_words_null_context_is_einval_without_a_device():
    L = api.load_library()
    assert L.ldpc_amd_set_symbol_unit(None, 4) == LDPC_AMD_EINVAL
    assert L.ldpc_amd_get_symbol_unit(None) == LDPC_AMD_EINVAL


def test_python_surface():
    assert callable(api.Context.set_symbol_unit)
    assert callable(api.Context.symbol_unit)
