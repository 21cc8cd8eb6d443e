"""Text columns (SZG_COL_STR), the parts that need no GPU: the C symbols and constants, the argument checks that
precede every device call, and the stand-alone program that runs the kernel's predicate and the heap's size arithmetic
(syzgydb_amd/csrc/column_str.h) on the host under the sanitizers.  test_gpu_text_columns.py has the device side."""
import ctypes
import os
import re
import shutil
import subprocess

from syzgydb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TEXT_SYMBOLS = ["szg_column_create_str", "szg_column_append_str", "szg_column_set_str", "szg_column_read_str",
                "szg_mask_where_str"]


def test_symbols_and_constants():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "syzgy_scan.h")).read()
    for name in TEXT_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared in the header" % name
    assert L.szg_abi_version() == 4
    assert (_lib.SZG_COL_F64, _lib.SZG_COL_U32, _lib.SZG_COL_STR) == (0, 1, 2)
    assert (_lib.SZG_STR_STARTS_WITH, _lib.SZG_STR_ENDS_WITH, _lib.SZG_STR_CONTAINS) == (6, 7, 8)
    assert _lib.SZG_STR_PATTERN_MAX == 256
    for name, value in (("SZG_COL_F64", 0), ("SZG_COL_U32", 1), ("SZG_COL_STR", 2), ("SZG_CMP_EQ", 0), ("SZG_CMP_GE", 5),
                        ("SZG_STR_STARTS_WITH", 6), ("SZG_STR_ENDS_WITH", 7), ("SZG_STR_CONTAINS", 8),
                        ("SZG_STR_PATTERN_MAX", 256)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name


def test_null_and_invalid_arguments_are_rejected_on_the_host():
    """Every check precedes device work: these calls run on a machine without a GPU, and *out stays untouched."""
    L = _lib.load()
    out = ctypes.c_void_p(0x1234)
    text = (ctypes.c_uint8 * 4)(*b"abcd")
    offsets = (ctypes.c_uint64 * 3)(0, 2, 4)
    bits = (ctypes.c_uint64 * 1)(3)
    assert L.szg_column_create_str(None, text, offsets, None, 2, ctypes.byref(out)) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error()
    assert L.szg_column_create_str(None, text, None, bits, 2, ctypes.byref(out)) == _lib.SZG_E_INVALID
    assert L.szg_column_append_str(None, text, offsets, None, 2) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error()
    assert L.szg_column_set_str(None, 0, text, 4) == _lib.SZG_E_INVALID
    assert L.szg_column_read_str(None, 0, 0, None, None, 0, None) == _lib.SZG_E_INVALID
    assert L.szg_mask_where_str(None, _lib.SZG_STR_CONTAINS, text, 4, None, ctypes.byref(out)) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error()
    for op in (-1, 9, 100):
        assert L.szg_mask_where_str(None, op, text, 4, None, ctypes.byref(out)) == _lib.SZG_E_INVALID
        assert b"operator" in L.szg_last_error()
    long_constant = (ctypes.c_uint8 * 257)()
    assert L.szg_mask_where_str(None, _lib.SZG_CMP_EQ, long_constant, 257, None, ctypes.byref(out)) == _lib.SZG_E_UNSUPPORTED
    assert L.szg_mask_where_str(None, _lib.SZG_CMP_EQ, None, 1, None, ctypes.byref(out)) == _lib.SZG_E_INVALID
    # the generic create keeps refusing the kind
    assert L.szg_column_create(None, _lib.SZG_COL_STR, text, None, 1, ctypes.byref(out)) == _lib.SZG_E_INVALID
    # offsets that decrease, or that do not start at 0
    for bad in ((0, 3, 2), (1, 2, 4)):
        offs = (ctypes.c_uint64 * 3)(*bad)
        assert L.szg_column_create_str(None, text, offs, None, 2, ctypes.byref(out)) == _lib.SZG_E_INVALID
        assert b"offsets" in L.szg_last_error()
        assert L.szg_column_append_str(None, text, offs, None, 2) == _lib.SZG_E_INVALID
        assert b"offsets" in L.szg_last_error()
    assert out.value == 0x1234


def test_standalone_predicate_program_is_clean_under_sanitizers(tmp_path):
    """The predicate the kernel runs and the heap's size arithmetic (column_str.h), in a stand-alone program with its
    own main, plain g++: every value of length 0..6 over {0x00, 'a', 0xff} against every constant of length 0..4, all
    nine operators, at all 16 alignments of a heap allocated exactly as the library sizes it, flanked by bytes that
    would complete a match; long values and constants; the split over parts, the 4 GiB refusal, bad offsets."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_column_str.cpp"
    exe = str(tmp_path / "test_column_str")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_column_str.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "column str ok" in done.stdout
