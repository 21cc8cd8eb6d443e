"""Vectors out to device memory and queries from it, the parts that need no GPU: the three C symbols, the unchanged
ABI and descriptor, the NULL refusals, and the Python methods' argument checks -- all of which come before the library
(or a card) is touched.  test_gpu_fetch_dev.py and test_gpu_search_dev.py have the device side."""
import ctypes
import os
import re

import pytest

from syzgydb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x7F0000001000
NAMES = ("szg_index_fetch_rows_dev", "szg_search_topk_dev", "szg_search_radius_dev")


class FakeDevice:
    def __init__(self, index):
        self.index = index


class FakeTensor:
    """torch's surface as dev_vectors reads it (strides in elements)."""

    def __init__(self, shape, dtype, strides, is_cuda=True, index=0, ptr=PTR):
        self.shape, self.dtype, self._strides, self.is_cuda, self.device, self._ptr = shape, dtype, strides, is_cuda, FakeDevice(index), ptr

    def stride(self):
        return self._strides

    def data_ptr(self):
        return self._ptr


def test_symbols_abi_and_struct():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "syzgy_scan.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS
        assert re.search(r"^int %s\s*\(" % name, hdr, flags=re.M)
    assert L.szg_abi_version() == 4
    assert ctypes.sizeof(_lib.SzgDevVectors) == 32
    assert "none of the queries" not in hdr
    assert re.search(r"szg_index_fetch_rows_dev WRITES through", hdr)   # (the descriptor's const is the ingest's)


def test_null_handle_and_null_descriptor_are_refused():
    L = _lib.load()
    d = _lib.SzgDevVectors(PTR, _lib.SZG_SRC_F32, 0, 1, 4)
    rows = (ctypes.c_uint64 * 1)(0)
    out_rows, out_dist = (ctypes.c_uint64 * 4)(), (ctypes.c_double * 4)()
    count, off, radii = (ctypes.c_int32 * 1)(), (ctypes.c_uint64 * 2)(), (ctypes.c_double * 1)(1.0)
    fake = ctypes.c_void_p(PTR)   # (never read: the descriptor is looked at first)
    calls = [
        lambda h, dd: L.szg_index_fetch_rows_dev(h, rows, 0, 1, dd),
        lambda h, dd: L.szg_index_fetch_rows_dev(h, None, 0, 1, dd),
        lambda h, dd: L.szg_search_topk_dev(h, dd, None, 1, 1, None, 0, out_rows, out_dist, count),
        lambda h, dd: L.szg_search_radius_dev(h, dd, None, 1, radii, None, 0, out_rows, out_dist, 4, off),
    ]
    for call in calls:
        assert call(None, ctypes.byref(d)) == _lib.SZG_E_INVALID
        assert b"null argument" in L.szg_last_error()
        assert call(fake, None) == _lib.SZG_E_INVALID
        assert b"null argument" in L.szg_last_error()


def bare_index(dim=3):
    from syzgydb_amd.index import ScanIndex
    ix = object.__new__(ScanIndex)   # (no handle: the argument checks come first)
    ix.dim, ix._device0, ix._h = dim, 0, None
    return ix


def test_index_methods_check_before_the_library_is_called():
    import torch
    ix = bare_index()
    with pytest.raises(TypeError, match="read_rows"):
        ix.fetch_into(torch.zeros((4, 3)))
    with pytest.raises(TypeError, match="search_topk"):
        ix.search_topk_tensor(torch.zeros((4, 3)), 2)
    with pytest.raises(TypeError, match="search_radius_batch"):
        ix.search_radius_tensor(torch.zeros((4, 3)), 0.5)
    one_d = FakeTensor((3,), torch.float32, (1,))
    wide = FakeTensor((4, 5), torch.float32, (5, 1))
    for call in (lambda t: ix.fetch_into(t), lambda t: ix.search_topk_tensor(t, 2), lambda t: ix.search_radius_tensor(t, 0.5)):
        with pytest.raises(ValueError, match="2-D"):
            call(one_d)
        with pytest.raises(ValueError, match="dimensions"):
            call(wide)
        with pytest.raises(TypeError, match="dtype"):
            call(FakeTensor((4, 3), torch.int32, (3, 1)))
        with pytest.raises(ValueError, match="inner stride"):
            call(FakeTensor((4, 3), torch.float32, (1, 4)))


def test_collection_methods_check_before_the_library_is_called():
    import torch
    from syzgydb_amd import Collection
    c = object.__new__(Collection)   # (no handle either)
    c.DimensionCount, c._row_of, c._index, c._order_stale = 3, {7: 0}, bare_index(), False
    with pytest.raises(KeyError, match="record not found"):
        c.FetchVectors([7, 8], FakeTensor((2, 3), torch.float32, (3, 1)))
    with pytest.raises(TypeError, match="read_rows"):
        c.FetchVectors([7], torch.zeros((1, 3)))
    with pytest.raises(ValueError, match="dimension"):
        c.SearchBatchTensor(torch.zeros((2, 4)), K=1)
    with pytest.raises(ValueError, match="dimension"):
        c.SearchBatchTensor(torch.zeros(3), K=1)
    with pytest.raises(ValueError, match="listing mode"):
        c.SearchBatchTensor(torch.zeros((2, 3)))
    with pytest.raises(ValueError, match="exclusive"):
        c.SearchBatchTensor(torch.zeros((2, 3)), K=1, Filter=lambda i, m: True, Where=object())
    with pytest.raises(TypeError, match="search_topk"):
        c.SearchBatchTensor(torch.zeros((2, 3)), K=1)
