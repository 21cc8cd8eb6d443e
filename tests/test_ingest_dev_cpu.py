"""Ingest from device memory, the parts that need no GPU: the two C symbols and their struct, and
syzgydb_amd.index.dev_vectors -- the one function that turns a tensor into the szg_dev_vectors descriptor -- on fake
objects that carry __cuda_array_interface__, on fake tensors with torch's surface, and on CPU torch tensors.
test_gpu_ingest_dev.py has the device side."""
import ctypes
import os
import re

import pytest

from syzgydb_amd import _lib
from syzgydb_amd.index import dev_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x7F0000001000


class Cai:
    """An object with __cuda_array_interface__ and, optionally, a device."""

    def __init__(self, shape, typestr, strides=None, ptr=PTR, device="unset"):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "strides": strides,
                                         "version": 3}
        if device != "unset":
            self.device = device


class CupyDevice:
    def __init__(self, id):
        self.id = id


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


def fields(d):
    return (d.data, d.dtype, d.device, d.n_rows, d.row_stride)


def test_symbols_and_struct():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "syzgy_scan.h")).read()
    for name in ("szg_index_append_dev", "szg_index_overwrite_rows_dev"):
        assert hasattr(L, name) and name in _lib.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, hdr)
    assert L.szg_abi_version() == 4
    for i, name in enumerate(("SZG_SRC_F64", "SZG_SRC_F32", "SZG_SRC_F16", "SZG_SRC_BF16")):
        assert getattr(_lib, name) == i and re.search(r"#define %s %d\b" % (name, i), hdr)
    body = re.search(r"typedef struct szg_dev_vectors \{(.*?)\} szg_dev_vectors;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    assert names == [f[0] for f in _lib.SzgDevVectors._fields_]
    assert ctypes.sizeof(_lib.SzgDevVectors) == 32
    # a null handle or a null descriptor is refused before anything is read
    d = _lib.SzgDevVectors(PTR, _lib.SZG_SRC_F32, 0, 1, 4)
    rows = (ctypes.c_uint64 * 1)(0)
    assert L.szg_index_append_dev(None, ctypes.byref(d), None, 1) == _lib.SZG_E_INVALID
    assert L.szg_index_overwrite_rows_dev(None, rows, ctypes.byref(d), None, 1) == _lib.SZG_E_INVALID


@pytest.mark.parametrize("typestr,code,es", [("<f8", _lib.SZG_SRC_F64, 8), ("<f4", _lib.SZG_SRC_F32, 4), ("<f2", _lib.SZG_SRC_F16, 2)])
def test_array_interface(typestr, code, es):
    # C-contiguous (strides None), the device taken from the argument, an int attribute, a cupy-style and a torch-style one
    assert fields(dev_vectors(Cai((7, 3), typestr), 3, device=2)) == (PTR, code, 2, 7, 3)
    assert fields(dev_vectors(Cai((7, 3), typestr, device=1), 3)) == (PTR, code, 1, 7, 3)
    assert fields(dev_vectors(Cai((7, 3), typestr, device=CupyDevice(3)), 3, device=0)) == (PTR, code, 3, 7, 3)
    assert fields(dev_vectors(Cai((7, 3), typestr, device=FakeDevice(1)), 3)) == (PTR, code, 1, 7, 3)
    # explicit strides in bytes: dense, and a column slice of a matrix 10 wide
    assert fields(dev_vectors(Cai((7, 3), typestr, strides=(3 * es, es)), 3, device=0)) == (PTR, code, 0, 7, 3)
    assert fields(dev_vectors(Cai((7, 3), typestr, strides=(10 * es, es), ptr=PTR + es), 3, device=0)) == (PTR + es, code, 0, 7, 10)
    # one row, no row: the row stride is never used and is reported as dim
    assert fields(dev_vectors(Cai((1, 3), typestr, strides=(0, es)), 3, device=0)) == (PTR, code, 0, 1, 3)
    assert fields(dev_vectors(Cai((0, 3), typestr, ptr=0), 3, device=0)) == (None, code, 0, 0, 3)
    # refusals
    with pytest.raises(ValueError, match="inner stride"):
        dev_vectors(Cai((7, 3), typestr, strides=(6 * es, 2 * es)), 3, device=0)
    with pytest.raises(ValueError, match="row stride"):
        dev_vectors(Cai((7, 3), typestr, strides=(2 * es, es)), 3, device=0)
    with pytest.raises(ValueError, match="row stride"):
        dev_vectors(Cai((7, 3), typestr, strides=(0, es)), 3, device=0)   # (a broadcast row)
    with pytest.raises(ValueError, match="negative"):
        dev_vectors(Cai((7, 3), typestr, strides=(-3 * es, es)), 3, device=0)
    with pytest.raises(ValueError, match="negative"):
        dev_vectors(Cai((7, 3), typestr, strides=(3 * es, -es)), 3, device=0)
    with pytest.raises(ValueError, match="multiples of the element size"):
        dev_vectors(Cai((7, 3), typestr, strides=(3 * es + 1, es)), 3, device=0)
    with pytest.raises(ValueError, match="dimensions"):
        dev_vectors(Cai((7, 3), typestr), 4, device=0)
    with pytest.raises(ValueError, match="2-D"):
        dev_vectors(Cai((7,), typestr), 7, device=0)
    with pytest.raises(ValueError, match="2-D"):
        dev_vectors(Cai((7, 3, 1), typestr), 3, device=0)
    with pytest.raises(ValueError, match="which device"):
        dev_vectors(Cai((7, 3), typestr), 3)


@pytest.mark.parametrize("typestr", ["<i4", "<u2", "<f16", ">f4", "|b1", "<c8"])
def test_array_interface_dtype_refused(typestr):
    with pytest.raises(TypeError, match="typestr"):
        dev_vectors(Cai((7, 3), typestr), 3, device=0)


def test_not_an_array():
    for obj in ([[1.0, 2.0, 3.0]], None, 3.5, b"abc"):
        with pytest.raises(TypeError, match="__cuda_array_interface__"):
            dev_vectors(obj, 3, device=0)


def test_tensor_surface():
    """torch's surface on a stand-in (no card here): the four dtypes by their names, strides in elements, the device's
    index before the argument."""
    import torch
    for dtype, code in ((torch.float64, _lib.SZG_SRC_F64), (torch.float32, _lib.SZG_SRC_F32), (torch.float16, _lib.SZG_SRC_F16),
                        (torch.bfloat16, _lib.SZG_SRC_BF16)):
        assert fields(dev_vectors(FakeTensor((5, 3), dtype, (3, 1), index=1), 3, device=0)) == (PTR, code, 1, 5, 3)
        assert fields(dev_vectors(FakeTensor((5, 3), dtype, (8, 1), index=None), 3, device=2)) == (PTR, code, 2, 5, 8)
    for dtype in (torch.int32, torch.int8, torch.bool, torch.complex64, torch.uint8):
        with pytest.raises(TypeError, match="dtype"):
            dev_vectors(FakeTensor((5, 3), dtype, (3, 1)), 3)
    f32 = torch.float32
    with pytest.raises(ValueError, match="inner stride"):
        dev_vectors(FakeTensor((5, 3), f32, (1, 5)), 3)           # (a transpose)
    with pytest.raises(ValueError, match="inner stride"):
        dev_vectors(FakeTensor((5, 3), f32, (6, 2)), 3)           # (every other column)
    with pytest.raises(ValueError, match="row stride"):
        dev_vectors(FakeTensor((5, 3), f32, (0, 1)), 3)           # (an expanded row)
    with pytest.raises(ValueError, match="negative"):
        dev_vectors(FakeTensor((5, 3), f32, (-3, 1)), 3)
    with pytest.raises(ValueError, match="dimensions"):
        dev_vectors(FakeTensor((5, 4), f32, (4, 1)), 3)
    with pytest.raises(ValueError, match="2-D"):
        dev_vectors(FakeTensor((5,), f32, (1,)), 5)
    with pytest.raises(ValueError, match="which device"):
        dev_vectors(FakeTensor((5, 3), f32, (3, 1), index=None), 3)


def test_cpu_tensors_are_refused_with_a_pointer_to_the_host_path():
    import torch
    for dtype in (torch.float64, torch.float32, torch.float16, torch.bfloat16, torch.int32):
        t = torch.zeros((4, 3), dtype=dtype)
        with pytest.raises(TypeError, match="append_vectors"):
            dev_vectors(t, 3, device=0)
    with pytest.raises(TypeError, match="append_vectors"):
        dev_vectors(torch.zeros((4, 8))[:, 1:4], 3, device=0)   # (a CPU tensor is refused before its layout is read)
    # ... and the strides torch reports are what the stand-in of test_tensor_surface assumes
    t = torch.zeros((6, 8), dtype=torch.float16)
    assert t[:, 2:5].stride() == (8, 1) and t.t().stride() == (1, 8) and t[:, ::2].stride() == (8, 2)
    assert str(torch.bfloat16) == "torch.bfloat16" and str(t.dtype) == "torch.float16"


def test_methods_exist_and_check_before_the_library_is_called():
    from syzgydb_amd.index import ScanIndex
    ix = object.__new__(ScanIndex)   # (no handle: the argument checks come first)
    ix.dim, ix._device0 = 3, 0
    import torch
    with pytest.raises(TypeError, match="append_vectors"):
        ix.append_tensor(torch.zeros((4, 3)))
    with pytest.raises(TypeError, match="append_vectors"):
        ix.overwrite_tensor([0, 1, 2, 3], torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="source rows"):
        ix.overwrite_tensor([0, 1], FakeTensor((4, 3), torch.float32, (3, 1)), src_rows=[0, 1, 2])
    ix._h = None   # (its __del__ then has nothing to destroy)
