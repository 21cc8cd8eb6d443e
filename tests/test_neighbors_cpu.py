"""szg_index_neighbors without a device: the symbols, the refusals decided on the host, the join's plan."""
import ctypes
import re
from pathlib import Path

import pytest

from syzgydb_amd import _lib
from syzgydb_amd.index import join_plan

NAMES = ("szg_index_neighbors", "szg_index_neighbors_stats", "szg_debug_join_plan", "szg_debug_join_min_queries")


def test_symbols_are_declared_and_exported():
    header = (Path(__file__).resolve().parents[1] / "include" / "syzgy_scan.h").read_text()
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header) and name in _lib.EXPORTS and hasattr(L, name)
    assert L.szg_abi_version() == 4


def test_null_arguments_are_refused_before_any_device_work():
    L = _lib.load()
    out = (ctypes.c_uint64 * 4)()
    dist = (ctypes.c_double * 4)()
    assert L.szg_index_neighbors(None, None, 0, 1, 1, None, out, dist, None) == _lib.SZG_E_INVALID
    assert L.szg_index_neighbors_stats(None, None) == _lib.SZG_E_INVALID
    assert L.szg_debug_join_plan(768, 64, 60, 0, 256, 1 << 20, None) == _lib.SZG_E_INVALID
    assert L.szg_debug_join_min_queries(None, 64) == _lib.SZG_E_INVALID


@pytest.mark.parametrize("dim,qb,areg,lds", [(768, 64, 1, 2 * 12 * 1024), (1024, 64, 1, 32 * 1024),
                                              (1088, 64, 0, 32 * 1024 + 64 * 1088), (2112, 32, 0, 32 * 1024 + 32 * 2112),
                                              (4096, 16, 0, 32 * 1024 + 16 * 4096)])
def test_join_plan_query_block_and_lds(dim, qb, areg, lds):
    p = join_plan(dim, 1024, 60, cu_count=256, shard_rows=1 << 20)
    assert p["served"] == 1 and (p["qb"], p["areg"], p["lds_bytes"]) == (qb, areg, lds) and lds < 160 * 1024
    assert p["query_blocks"] == 1024 // qb and 1 <= p["m"] <= 16 and p["m"] < 60
    assert p["slices"] * p["tiles_per_slice"] >= (1 << 20) // 16 and p["slices"] <= 256


@pytest.mark.parametrize("dim", range(64, 4097, 64))
def test_join_plan_lds_stays_below_a_cu(dim):
    for rows, nq in ((17, 1), (1 << 20, 64), (3000, 1024)):
        p = join_plan(dim, nq, 47, masked=1, shard_rows=rows)
        assert p["served"] == 1 and p["lds_bytes"] < 160 * 1024 and p["masked"] == 1
        assert p["slices"] * p["tiles_per_slice"] >= (rows + 15) // 16 > (p["slices"] - 1) * p["tiles_per_slice"]


@pytest.mark.parametrize("dim,kp,nq", [(100, 60, 64), (4160, 60, 64), (768, 97, 64), (768, 60, 1025), (768, 60, 0), (768, 1, 64)])
def test_join_plan_refuses(dim, kp, nq):
    assert join_plan(dim, nq, kp)["served"] == 0
