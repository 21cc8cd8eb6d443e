"""Device-resident filter masks without a GPU: the new symbols are in the built library, reject null arguments
before any device work, and the ABI version has not moved."""
import ctypes

from syzgydb_amd import _lib

MASK_SYMBOLS = ["szg_mask_create", "szg_mask_create_rows", "szg_mask_combine", "szg_mask_count", "szg_mask_read",
                "szg_mask_destroy", "szg_search_topk_masked", "szg_search_radius_masked", "szg_index_mask_stats"]


def test_mask_symbols_resolve_and_abi_stays_4():
    L = _lib.load()
    for name in MASK_SYMBOLS:
        assert hasattr(L, name), "libsyzgy_scan.so does not export %s" % name
        assert name in _lib.EXPORTS
    assert L.szg_abi_version() == 4


def test_mask_null_arguments():
    L = _lib.load()
    h = ctypes.c_void_p()
    words = (ctypes.c_uint64 * 1)(1)
    q = (ctypes.c_double * 1)(0.0)
    rows = (ctypes.c_uint64 * 1)(0)
    dist = (ctypes.c_double * 1)(0.0)
    off = (ctypes.c_uint64 * 2)(0, 0)
    st = _lib.SzgMaskStats()
    assert L.szg_mask_create(None, words, ctypes.byref(h)) == _lib.SZG_E_INVALID
    assert L.szg_mask_create(None, None, None) == _lib.SZG_E_INVALID
    assert L.szg_mask_create_rows(None, rows, 1, ctypes.byref(h)) == _lib.SZG_E_INVALID
    assert not h
    for op in (_lib.SZG_MASK_AND, _lib.SZG_MASK_OR, _lib.SZG_MASK_ANDNOT, _lib.SZG_MASK_NOT):
        assert L.szg_mask_combine(op, None, None, ctypes.byref(h)) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error()
    assert L.szg_mask_read(None, words) == _lib.SZG_E_INVALID
    assert L.szg_mask_count(None) == 0
    assert L.szg_index_mask_stats(None, ctypes.byref(st)) == _lib.SZG_E_INVALID
    assert L.szg_search_topk_masked(None, q, 1, 1, None, 0, rows, dist, None) == _lib.SZG_E_INVALID
    assert L.szg_search_radius_masked(None, q, 1, q, None, 0, rows, dist, 1, off) == _lib.SZG_E_INVALID
    L.szg_mask_destroy(None)   # harmless
