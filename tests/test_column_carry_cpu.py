"""Columns carried across a compaction / reorder, the parts that need no GPU: the C symbols, the argument checks that
precede every device call, and the stand-alone program that runs the carry's index arithmetic
(syzgydb_amd/csrc/column_carry.h: the byte mover of the text heap's repack, the grouping by source part, the staging
windows, the capacities) on the host under the sanitizers.  test_gpu_column_carry.py has the device side."""
import ctypes
import os
import re
import shutil
import subprocess

from syzgydb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CARRY_SYMBOLS = ["szg_index_reorder_carry", "szg_index_compact_carry", "szg_column_get_info"]


def test_symbols():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "syzgy_scan.h")).read()
    for name in CARRY_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared in the header" % name
    assert L.szg_abi_version() == 4
    assert [f[0] for f in _lib.SzgColumnInfo._fields_] == ["kind", "rows", "device_bytes", "heap_used", "heap_capacity"]
    assert ctypes.sizeof(_lib.SzgColumnInfo) == 40


def test_null_arguments_are_rejected_on_the_host():
    L = _lib.load()
    info = _lib.SzgColumnInfo()
    assert L.szg_index_reorder_carry(None, None, 0, None, 0, None, 0) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error()
    assert L.szg_index_compact_carry(None, None, None, None, 0, None, 0) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error()
    assert L.szg_column_get_info(None, ctypes.byref(info)) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error()


def test_standalone_carry_program_is_clean_under_sanitizers(tmp_path):
    """column_carry.h in a stand-alone program with its own main, plain g++: the byte mover against memcpy for values
    of length 0, 1, 3, 4, 5, 15, 16, 17, 33, 300 and 4998 at every old alignment, listed forwards, in reverse and with
    gaps, on heaps allocated exactly as the library sizes them, the last value ending at the used bytes; the grouping
    and the windows for 1, 2 and 3 parts under a row-by-row interleaved list; the capacity arithmetic."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_column_carry.cpp"
    exe = str(tmp_path / "test_column_carry")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_column_carry.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "column carry ok" in done.stdout
