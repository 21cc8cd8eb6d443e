"""Bulk mutations without a GPU: the new symbols are in the built library and in the header, the entry points reject
null arguments before any device work, the ABI version has not moved, and the host-only plan -- the checks every bulk
call makes on its list, and the list's split over shards -- answers as documented.  The plan is the one part that reads
a caller's list unchecked, so a stand-alone program (tests/cpp/test_bulk_plan.cpp, plain g++, its own main) runs it over
malformed lists under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from syzgydb_amd import SzgError, _lib, bulk_plan, reorder_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BULK_SYMBOLS = ["szg_index_overwrite_rows", "szg_index_overwrite_rows_f64", "szg_index_tombstone_rows",
                "szg_index_tombstone_mask", "szg_column_set_rows", "szg_debug_bulk_plan"]


def test_bulk_symbols_resolve_and_abi_stays_4():
    L = _lib.load()
    for name in BULK_SYMBOLS:
        assert hasattr(L, name), "libsyzgy_scan.so does not export %s" % name
        assert name in _lib.EXPORTS
    assert L.szg_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "syzgy_scan.h")).read()
    assert "#define SZG_ABI_VERSION 4" in header
    for name in BULK_SYMBOLS:
        assert name + "(" in header


def test_bulk_null_arguments():
    L = _lib.load()
    rows = (ctypes.c_uint64 * 2)(0, 1)
    data = (ctypes.c_uint8 * 64)()
    vec = (ctypes.c_double * 8)()
    out = ctypes.c_uint64(7)
    for rc in (L.szg_index_overwrite_rows(None, rows, data, 2), L.szg_index_overwrite_rows(None, None, None, 0),
               L.szg_index_overwrite_rows_f64(None, rows, vec, 2), L.szg_index_tombstone_rows(None, rows, 2, ctypes.byref(out)),
               L.szg_index_tombstone_mask(None, None, ctypes.byref(out)),
               L.szg_column_set_rows(None, rows, ctypes.cast(vec, ctypes.c_void_p), None, 2)):
        assert rc == _lib.SZG_E_INVALID
        assert b"null" in L.szg_last_error()
    assert out.value == 7
    assert L.szg_debug_bulk_plan(4, 0, None, 2, 1, 0, None, None, None, None, None) == _lib.SZG_E_INVALID
    assert L.szg_debug_bulk_plan(4, 0, rows, 2, 0, 0, None, None, None, None, None) == _lib.SZG_E_INVALID


@pytest.mark.parametrize("shards", [1, 2, 3])
def test_plan_split_matches_the_shard_boundaries(shards):
    n = 200
    counts = reorder_plan(n, np.arange(n), n_shards=shards)   # a load's split: boundaries at multiples of 64
    first = np.concatenate([[0], np.cumsum(counts)])[:shards]
    assert all(int(f) % 64 == 0 for f, c in zip(first, counts) if c)
    rng = np.random.default_rng(5 + shards)
    edges = [0, 63, 64, 127, 128, 199]
    rows = rng.permutation(np.concatenate([edges, rng.permutation(np.setdiff1d(np.arange(n), edges))[:144]]))
    plan = bulk_plan(n, rows, n_shards=shards)
    assert len(plan) == shards
    seen = []
    for s, part in enumerate(plan):
        want_src = [i for i, r in enumerate(rows) if first[s] <= r < first[s] + counts[s]]
        assert part["source"] == want_src                                    # the caller's order, positions kept
        assert part["local"] == [int(rows[i] - first[s]) for i in want_src]  # entry i's data is found through source
        if want_src:
            assert part["words"] == (min(part["local"]) // 64, max(part["local"]) // 64)
        else:
            assert part["words"] is None
        seen += want_src
    assert sorted(seen) == list(range(rows.size))


def test_plan_empty_list():
    assert bulk_plan(200, []) == [{"local": [], "source": [], "words": None}]
    assert bulk_plan(200, [], n_shards=3) == [{"local": [], "source": [], "words": None}] * 3
    assert bulk_plan(0, [], allow_duplicates=True) == [{"local": [], "source": [], "words": None}]


@pytest.mark.parametrize("shards", [1, 2, 3])
@pytest.mark.parametrize("rows,code,text", [
    ([3, 3], _lib.SZG_E_INVALID, "row listed twice"),
    ([0, 64, 5, 64], _lib.SZG_E_INVALID, "row listed twice"),
    ([0, 200], _lib.SZG_E_RANGE, "row out of range"),          # row == n_rows
    ([2 ** 64 - 1], _lib.SZG_E_RANGE, "row out of range"),
    ([3, 3, 200], _lib.SZG_E_RANGE, "row out of range"),
])
def test_plan_rejects(rows, code, text, shards):
    with pytest.raises(SzgError) as e:
        bulk_plan(200, rows, n_shards=shards)
    assert e.value.code == code and text in str(e.value)


def test_plan_tombstone_form_accepts_duplicates_but_not_range_faults():
    plan = bulk_plan(200, [3, 3, 199, 3], allow_duplicates=True)
    assert plan[0]["local"] == [3, 3, 199, 3] and plan[0]["source"] == [0, 1, 2, 3]
    for bad in (200, 2 ** 64 - 1):
        with pytest.raises(SzgError) as e:
            bulk_plan(200, [3, bad], allow_duplicates=True)
        assert e.value.code == _lib.SZG_E_RANGE and "row out of range" in str(e.value)


def test_plan_removes_the_row_base():
    plan = bulk_plan(200, [1000 + 130, 1000, 1000 + 63], n_shards=2, row_base=1000)
    assert plan[0] == {"local": [0, 63], "source": [1, 2], "words": (0, 0)}
    assert plan[1] == {"local": [2], "source": [0], "words": (0, 0)}
    for bad in (999, 1200):
        with pytest.raises(SzgError) as e:
            bulk_plan(200, [bad], row_base=1000)
        assert e.value.code == _lib.SZG_E_RANGE


def test_plan_tombstone_word_ranges():
    rows = [0, 63, 64, 129]
    assert bulk_plan(200, rows, allow_duplicates=True)[0]["words"] == (0, 2)
    two = bulk_plan(200, rows, n_shards=2, allow_duplicates=True)    # 128 + 72 rows
    assert two[0]["words"] == (0, 1) and two[1]["words"] == (0, 0) and two[1]["local"] == [1]
    assert bulk_plan(200, [129, 70], allow_duplicates=True)[0]["words"] == (1, 2)


def test_standalone_plan_program_is_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_bulk_plan.cpp"
    exe = str(tmp_path / "test_bulk_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_bulk_plan.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "bulk plan ok" in done.stdout
