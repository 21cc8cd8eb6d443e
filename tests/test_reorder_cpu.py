"""Compaction and reorder of the resident rows without a GPU: the new symbols are in the built library, the entry
points reject null arguments before any device work, the ABI version has not moved, and the host-only plan -- the
checks szg_index_reorder makes on its list, and the split over shards -- answers as documented.  The plan is the one
part that reads a caller's list unchecked, so a stand-alone program (tests/cpp/test_reorder_plan.cpp, plain g++, its
own main) runs it over malformed lists under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from syzgydb_amd import SzgError, _lib, reorder_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REORDER_SYMBOLS = ["szg_index_reorder", "szg_index_compact", "szg_debug_reorder_plan"]


def test_reorder_symbols_resolve_and_abi_stays_4():
    L = _lib.load()
    for name in REORDER_SYMBOLS:
        assert hasattr(L, name), "libsyzgy_scan.so does not export %s" % name
        assert name in _lib.EXPORTS
    assert L.szg_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "syzgy_scan.h")).read()
    assert "#define SZG_ABI_VERSION 4" in header
    for name in REORDER_SYMBOLS:
        assert name + "(" in header


def test_reorder_null_arguments():
    L = _lib.load()
    rows = (ctypes.c_uint64 * 2)(0, 1)
    out = ctypes.c_uint64(7)
    assert L.szg_index_reorder(None, rows, 2, None, 0) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error()
    assert L.szg_index_reorder(None, None, 0, None, 0) == _lib.SZG_E_INVALID
    assert L.szg_index_compact(None, None, ctypes.byref(out), None, 0) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error()
    assert out.value == 7
    assert L.szg_debug_reorder_plan(4, None, None, 2, 1, None) == _lib.SZG_E_INVALID
    assert L.szg_debug_reorder_plan(4, None, rows, 2, 0, None) == _lib.SZG_E_INVALID


def test_plan_good_list():
    assert reorder_plan(100, [99, 0, 64, 63, 5]) == [5]
    assert reorder_plan(100, np.arange(100)[::-1], n_shards=2) == [64, 36]
    live = np.ones(100, bool)
    live[[3, 64]] = False
    assert reorder_plan(100, [2, 4, 63, 65], live=live) == [4]


@pytest.mark.parametrize("rows,code,text", [
    ([3, 3], _lib.SZG_E_INVALID, "row listed twice"),
    ([0, 64, 5, 64], _lib.SZG_E_INVALID, "row listed twice"),
    ([0, 100], _lib.SZG_E_RANGE, "row out of range"),          # row == n_rows
    ([2 ** 64 - 1], _lib.SZG_E_RANGE, "row out of range"),
    (list(range(100)) + [5], _lib.SZG_E_INVALID, "row listed twice"),
    (list(range(100)) + [100], _lib.SZG_E_RANGE, "row out of range"),
])
def test_plan_rejects(rows, code, text):
    with pytest.raises(SzgError) as e:
        reorder_plan(100, rows)
    assert e.value.code == code and text in str(e.value)


def test_plan_dead_row():
    live = np.ones(130, bool)
    live[[0, 64, 129]] = False
    for dead in (0, 64, 129):
        with pytest.raises(SzgError) as e:
            reorder_plan(130, [1, dead], live=live)
        assert e.value.code == _lib.SZG_E_INVALID and "tombstoned" in str(e.value)
    assert reorder_plan(130, [128, 1, 65], live=live) == [3]


def test_plan_empty_list():
    assert reorder_plan(100, []) == [0]
    assert reorder_plan(100, [], n_shards=3) == [0, 0, 0]
    assert reorder_plan(0, []) == [0]


@pytest.mark.parametrize("n,shards,want", [
    (1, 1, [1]), (1, 2, [1, 0]), (1, 3, [1, 0, 0]),
    (64, 1, [64]), (64, 2, [64, 0]), (64, 3, [64, 0, 0]),
    (65, 1, [65]), (65, 2, [64, 1]), (65, 3, [64, 1, 0]),
    (129, 1, [129]), (129, 2, [128, 1]), (129, 3, [64, 64, 1]),
])
def test_plan_shard_counts(n, shards, want):
    # (what szg_index_load's split gives for n rows: contiguous ranges, boundaries at multiples of 64)
    assert reorder_plan(200, np.arange(n, dtype=np.uint64) + 7, n_shards=shards) == want


def test_standalone_plan_program_is_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_reorder_plan.cpp"
    exe = str(tmp_path / "test_reorder_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_reorder_plan.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "reorder plan ok" in done.stdout
