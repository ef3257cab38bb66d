"""The ctypes signature table (cine_hip/_lib.py, ``_SIGS``) is parsed from include/cine_hip.h: the parser on synthetic header text, what it
refuses, literal spot checks of the table of the real header (one per type of the map), and the import without a header.  Runs without a GPU."""
import os
import shutil
import subprocess
import sys
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p

import pytest

from conftest import PKG
from cine_hip import _lib

P = c_void_p

SNIPPET = """
/* a block comment with a prototype inside: int cine_fake(int);
 * over two lines */
#ifndef SNIPPET_H
#define SNIPPET_H
#include <stdint.h>
#define CINE_TWO_LINES (1 + \\
                        2)
#ifdef __cplusplus
extern "C" {
#endif
int cine_three_lines(const float* in, float* out,
                     int n, const uint8_t* mask, int h, const int* sizes, int w,
                     long count, void* stream);      // int cine_fake(int);
// int cine_fake(int);
size_t cine_bytes(void);
size_t cine_bytes_of(const int n, size_t each);
const char* cine_name_of(int which);
double cine_mixed(float a, double b, const void* const* table);
#ifdef __cplusplus
}
#endif
#endif /* SNIPPET_H */
"""


def test_parser_on_synthetic_header_text():
    assert _lib.parse_header(SNIPPET) == {
        "cine_three_lines": (c_int, [P, P, c_int, P, c_int, P, c_int, c_long, P]),
        "cine_bytes": (c_size_t, []),
        "cine_bytes_of": (c_size_t, [c_int, c_size_t]),
        "cine_name_of": (c_char_p, [c_int]),
        "cine_mixed": (c_double, [c_float, c_double, P]),
    }
    assert _lib.parse_header("") == {} and _lib.parse_header("int cine_empty();") == {"cine_empty": (c_int, [])}


@pytest.mark.parametrize("name,header", [
    ("cine_bad_u8", "int cine_bad_u8(const float* x, uint8_t m);"),
    ("cine_bad_unsigned", "int cine_bad_unsigned(unsigned n);"),
    ("cine_bad_string", "int cine_bad_string(const char* name);"),
    ("cine_bad_varargs", "int cine_bad_varargs(int n, ...);"),
    ("cine_bad_return", "float* cine_bad_return(int n);"),
    ("cine_bad_i64", "int cine_bad_i64(int64_t n);"),
    ("cine_bad_bool", "int cine_bad_bool(bool on);"),
    ("cine_bad_callback", "int cine_bad_callback(void (*done)(int, int), void* stream);"),
    ("cine_bad_array", "int cine_bad_array(int sizes[3]);"),
    ("cine_bad_struct", "int cine_bad_struct(struct dims d);"),
    ("cine_bad_void", "void cine_bad_void(int n);"),
    ("cine_bad_two_words", "int cine_bad_two_words(unsigned int n);"),
    ("cine_bad_body", "static inline int cine_bad_body(int n) { return n; }"),
    ("cine_bad_tail", "int cine_bad_tail(int n) __attribute__((cold));"),
    ("cine_twice", "int cine_twice(int n); int cine_twice(int n);"),
])
def test_parser_refuses_what_is_outside_the_convention(name, header):
    with pytest.raises(ValueError, match=name):
        _lib.parse_header(header)
    with pytest.raises(ValueError, match=name):                              # and between good neighbours
        _lib.parse_header("int cine_before(int n);\n" + header + "\nint cine_after(int n);")


def test_parser_refuses_a_statement_that_is_no_prototype():
    for header in ("typedef struct cine_ctx cine_ctx;", "int not_ours(int n);", "int cine_unfinished(int n"):
        with pytest.raises(ValueError):
            _lib.parse_header(header)


def test_spot_checks_on_the_real_header():
    """A second copy on purpose: these nine are written out by hand, one for each type the map knows, to guard the parser."""
    assert _lib._SIGS_ERROR is None
    expected = {
        "cine_version": (c_int, []),
        "cine_last_error": (c_char_p, []),
        "cine_profile_family_name": (c_char_p, [c_int]),
        "cine_fft1c": (c_int, [P, P, c_long, c_int, c_int, c_int, P]),
        "cine_image_dc": (c_int, [P, P, P, P, P, c_float, c_float, c_float, P, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P]),
        "cine_image_metrics": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_double, c_int, c_double, P, P, c_size_t, P]),
        "cine_dot_ws_bytes": (c_size_t, []),
        "cine_mwcnn_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int]),
        "cine_diag_counter": (c_long, [c_int, c_int]),
    }
    for name, sig in expected.items():
        assert _lib._SIGS[name] == sig, name
    with open(_lib.HEADER_PATH) as f:
        assert _lib.parse_header(f.read()) == _lib._SIGS
    assert sorted(_lib._SIGS) == _lib.declared_symbols()


def test_import_without_a_header(tmp_path):
    """The module imports where the header is absent (a copy of it two directories below an empty one); lib() then names the missing file."""
    home = tmp_path / "tree" / "cine_hip"
    home.mkdir(parents=True)
    shutil.copy(os.path.join(PKG, "cine_hip", "_lib.py"), home / "_lib.py")
    header = tmp_path / "include" / "cine_hip.h"
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import _lib\n"
            "assert _lib.HEADER_PATH == sys.argv[2], _lib.HEADER_PATH\n"
            "assert _lib._SIGS == {}\n"
            "try:\n"
            "    _lib.lib()\n"
            "except _lib.CineHipError as e:\n"
            "    assert sys.argv[2] in str(e), str(e)\n"
            "    print('refused')\n")
    out = subprocess.run([sys.executable, "-c", code, str(home), str(header)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "refused", out.stderr


def test_an_unparsable_header_surfaces_from_lib(monkeypatch, tmp_path):
    bad = tmp_path / "cine_hip.h"
    bad.write_text("int cine_version(void);\nint cine_bad_unsigned(unsigned n);\n")
    monkeypatch.setattr(_lib, "HEADER_PATH", str(bad))
    sigs, error = _lib._load_sigs()
    assert sigs == {} and str(bad) in error and "cine_bad_unsigned" in error
    monkeypatch.setattr(_lib, "_SIGS_ERROR", error)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.CineHipError, match="cine_bad_unsigned"):
        _lib.lib()
