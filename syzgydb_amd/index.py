"""ScanIndex: thin Python handle over the C ABI of include/syzgy_scan.h.

One ScanIndex == one szg_index == the HBM mirror of one Collection's packed
vectors.  All compute happens in libsyzgy_scan.so (HIP, gfx950).
"""
import contextlib
import ctypes
import os
import weakref

import numpy as np

from . import _lib, regex_dfa
from ._lib import (SZG_COSINE, SZG_EUCLIDEAN, SzgColumnInfo, SzgError, SzgMaskStats, SzgScanPlan, SzgStats,  # noqa: F401
                   check)
from .where import _bytes


def _u8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _u64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def _f64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def pack_allow_bits(mask):
    """bool[n_rows] (or [n_queries, n_rows]) -> uint64 words, bit r of word r//64."""
    m = np.atleast_2d(np.asarray(mask, dtype=bool))
    nq, n = m.shape
    words = (n + 63) // 64
    padded = np.zeros((nq, words * 64), dtype=np.uint8)
    padded[:, :n] = m
    packed = np.packbits(padded, axis=1, bitorder="little")
    return np.ascontiguousarray(packed).view(np.uint64).reshape(nq, words)


_TORCH_SRC = {"torch.float64": _lib.SZG_SRC_F64, "torch.float32": _lib.SZG_SRC_F32, "torch.float16": _lib.SZG_SRC_F16,
              "torch.bfloat16": _lib.SZG_SRC_BF16}
_CAI_SRC = {"<f8": _lib.SZG_SRC_F64, "<f4": _lib.SZG_SRC_F32, "<f2": _lib.SZG_SRC_F16}   # (no typestr names bfloat16)
_SRC_BYTES = (8, 4, 2, 2)


def dev_vectors(t, dim, device=None):
    """The szg_dev_vectors descriptor of a 2-D array of vectors in device memory: a torch tensor (duck-typed on
    data_ptr, dtype, shape, stride, device and is_cuda; torch is not imported) or any object with
    __cuda_array_interface__.  Nothing is copied and no device is touched; the caller keeps `t` alive.
    The rules: float64, float32, float16 or bfloat16 (else TypeError); shape (n, dim); inner stride 1; a row stride of
    at least dim (larger: a column slice of a wider tensor); no negative stride (else ValueError).  A CPU tensor is a
    TypeError: host memory goes through append_vectors / overwrite_vectors.  device: the ordinal to assume where the
    object does not name one (the array interface has no such field)."""
    if hasattr(t, "data_ptr"):
        if not getattr(t, "is_cuda", False):
            raise TypeError("a CPU tensor is host memory: use append_vectors / overwrite_vectors (or AddDocuments with "
                            "an array), which take float64 on the host")
        dtype = _TORCH_SRC.get(str(t.dtype))
        if dtype is None:
            raise TypeError("tensor dtype %s: float64, float32, float16 or bfloat16 expected" % (t.dtype,))
        shape = tuple(int(x) for x in t.shape)
        strides = tuple(int(x) for x in t.stride())
        ptr = int(t.data_ptr())
        if getattr(t.device, "index", None) is not None:
            device = t.device.index
    elif hasattr(t, "__cuda_array_interface__"):
        cai = t.__cuda_array_interface__
        dtype = _CAI_SRC.get(cai["typestr"])
        if dtype is None:
            raise TypeError("array typestr %r: '<f8', '<f4' or '<f2' expected" % (cai["typestr"],))
        shape = tuple(int(x) for x in cai["shape"])
        es = _SRC_BYTES[dtype]
        if cai.get("strides") is None:   # C-contiguous
            strides = tuple(int(np.prod(shape[i + 1:], dtype=np.int64)) for i in range(len(shape)))
        else:
            if any(int(s) % es for s in cai["strides"]):
                raise ValueError("array strides %r are not multiples of the element size %d" % (cai["strides"], es))
            strides = tuple(int(s) // es for s in cai["strides"])
        ptr = int(cai["data"][0] or 0)
        d = getattr(t, "device", None)
        d = d if isinstance(d, int) else getattr(d, "id", getattr(d, "index", None))
        if d is not None:
            device = int(d)
    else:
        raise TypeError("vectors in device memory: a torch tensor or an object with __cuda_array_interface__ expected")
    if len(shape) != 2:
        raise ValueError("a 2-D array of vectors expected, got shape %r" % (shape,))
    n, width = shape
    if width != dim:
        raise ValueError("vector size does not match the expected number of dimensions: expected %d, got %d" % (dim, width))
    if any(s < 0 for s in strides):
        raise ValueError("negative strides %r" % (strides,))
    if strides[1] != 1:
        raise ValueError("the inner stride is %d: the elements of a vector must be contiguous" % strides[1])
    row_stride = strides[0]
    if n <= 1:
        row_stride = max(row_stride, dim)   # (no second row: whatever stride the array reports is never used)
    elif row_stride < dim:
        raise ValueError("the row stride %d is smaller than the dimension %d: rows overlap" % (row_stride, dim))
    if device is None:
        raise ValueError("the array does not say which device it lies on")
    return _lib.SzgDevVectors(ptr or None, dtype, int(device), n, row_stride)


class ScanMask:
    """A filter mask that lives on the card (szg_mask): made once per (filter, collection version) by
    ScanIndex.mask / mask_rows or composed from other masks with & | ~ and andnot, then passed to the searches as
    masks=.  It keeps its ScanIndex alive; the index closes the masks it still holds before it closes itself.  A load
    or an append makes older masks stale: searches with them raise SzgError (SZG_E_INVALID), read() and count still
    work."""

    def __init__(self, index, handle, words):
        self._index = index
        self._L = index._L
        self._h = handle
        self._words = words   # per mask, as of its creation
        index._masks[id(self)] = (weakref.ref(self), handle.value)

    def close(self):
        if self._h:
            # (a closed index has destroyed this mask already: the cycle collector clears weak references before it
            # runs __del__, so the index may not have seen this object, only its handle)
            if self._index._masks.pop(id(self), None) is not None:
                self._L.szg_mask_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _live(self):
        if not self._h:
            raise ValueError("mask is closed")
        return self._h

    @property
    def count(self):
        """Rows the mask allows (exact; tail bits are never set)."""
        return int(self._L.szg_mask_count(self._live()))

    def read(self):
        """The mask's words, uint64[ceil(rows / 64)], rows as of the mask's creation."""
        out = np.zeros(self._words, dtype=np.uint64)
        check(self._L.szg_mask_read(self._live(), _u64(out) if out.size else None), "szg_mask_read")
        return out

    def _combine(self, op, other):
        if other is not None and not isinstance(other, ScanMask):
            return NotImplemented
        h = ctypes.c_void_p()
        check(self._L.szg_mask_combine(op, self._live(), other._live() if other is not None else None, ctypes.byref(h)),
              "szg_mask_combine")
        return ScanMask(self._index, h, self._words)

    def __and__(self, other):
        return self._combine(_lib.SZG_MASK_AND, other)

    def __or__(self, other):
        return self._combine(_lib.SZG_MASK_OR, other)

    def andnot(self, other):
        """self & ~other."""
        return self._combine(_lib.SZG_MASK_ANDNOT, other)

    def __invert__(self):
        return self._combine(_lib.SZG_MASK_NOT, None)


_CMP_OPS = {"==": _lib.SZG_CMP_EQ, "!=": _lib.SZG_CMP_NE, "<": _lib.SZG_CMP_LT, "<=": _lib.SZG_CMP_LE,
            ">": _lib.SZG_CMP_GT, ">=": _lib.SZG_CMP_GE}
_TEXT = (bytes, bytearray, memoryview, str)


def _text(value):
    """One text value or constant as bytes: a str is encoded as the filter evaluator encodes it (where._bytes)."""
    return _bytes(value) if isinstance(value, str) else bytes(value)


def _text_arg(values, present):
    """A sequence of bytes / str / None as the *_str calls take it: (keep-alive array, bytes pointer, uint64
    offsets[n + 1], present).  None is an absent row unless `present` is given."""
    vals = [None if v is None else _text(v) for v in values]
    if present is None and any(v is None for v in vals):
        present = np.array([v is not None for v in vals], dtype=bool)
    offsets = np.zeros(len(vals) + 1, dtype=np.uint64)
    if vals:
        np.cumsum([0 if v is None else len(v) for v in vals], out=offsets[1:])
    data = np.frombuffer(b"".join(v for v in vals if v is not None), dtype=np.uint8)
    return data, (_u8(data) if data.size else None), offsets, present


class ScanColumn:
    """A metadata column that lives on the card beside the rows (szg_column): one value and one present bit per row,
    float64 values (kind F64), uint32 codes of a dictionary the caller owns (kind U32), or the strings themselves as
    bytes (kind STR, a text column).  Made by ScanIndex.column / text_column; where / isin / codes / startswith /
    endswith / contains / present compare it against constants ON THE DEVICE and return a ScanMask.  Index appends
    leave it short until append() catches up; a load, a synth, and a reorder or a compaction that moves rows and is not
    given the column in carry= make it stale (every call but rows / read / info / close then raises SzgError,
    SZG_E_INVALID)."""

    def __init__(self, index, handle, kind):
        self._index = index
        self._L = index._L
        self._h = handle
        self.kind = kind
        self._dtype = np.float64 if kind == _lib.SZG_COL_F64 else np.uint32
        index._columns[id(self)] = (weakref.ref(self), handle.value)

    def close(self):
        if self._h:
            if self._index._columns.pop(id(self), None) is not None:   # (as ScanMask.close)
                self._L.szg_column_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _live(self):
        if not self._h:
            raise ValueError("column is closed")
        return self._h

    @staticmethod
    def _present_arg(present, n):
        """present -> (keep-alive array, pointer): None = all present; bool[n] or uint64 words, bit i = row i."""
        if present is None:
            return None, None
        a = np.asarray(present)
        if a.dtype != np.uint64:
            a = pack_allow_bits(a.reshape(-1).astype(bool))[0]
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        if a.size != (n + 63) // 64:
            raise ValueError("present has %d words, %d rows need %d" % (a.size, n, (n + 63) // 64))
        return a, (_u64(a) if a.size else None)

    def append(self, values, present=None):
        """Rows behind the column's last (the index holds them already); present refers to THESE rows."""
        if self.kind == _lib.SZG_COL_STR:
            data, dp, offsets, present = _text_arg(values, present)
            keep, pp = self._present_arg(present, offsets.size - 1)
            check(self._L.szg_column_append_str(self._live(), dp, _u64(offsets), pp, offsets.size - 1), "szg_column_append_str")
            del keep, data
            return
        v = np.ascontiguousarray(values, dtype=self._dtype).reshape(-1)
        keep, pp = self._present_arg(present, v.size)
        check(self._L.szg_column_append(self._live(), v.ctypes.data_as(ctypes.c_void_p) if v.size else None, pp, v.size),
              "szg_column_append")
        del keep

    def set(self, row, value):
        """One row's value; None marks it absent."""
        if self.kind == _lib.SZG_COL_STR:
            b = None if value is None else _text(value)
            buf = None if b is None else (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")
            check(self._L.szg_column_set_str(self._live(), int(row), buf, len(b) if b is not None else 0), "szg_column_set_str")
            return
        v = None if value is None else np.asarray([value], dtype=self._dtype)
        check(self._L.szg_column_set(self._live(), int(row), v.ctypes.data_as(ctypes.c_void_p) if v is not None else None),
              "szg_column_set")

    def set_rows(self, rows, values, present=None):
        """Many rows' values in one call (F64 and U32 columns; a text column raises SzgError, SZG_E_INVALID: its values
        go through set(), row by row).  values[i] belongs to rows[i]; present: None = every entry, bool per entry or
        uint64 words -- an absent entry marks its row absent and its value is ignored.  A row out of range or listed
        twice refuses the whole call."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        v = np.ascontiguousarray(values, dtype=self._dtype).reshape(-1)
        if v.size != r.size:
            raise ValueError("%d values for %d rows" % (v.size, r.size))
        keep, pp = self._present_arg(present, r.size)
        check(self._L.szg_column_set_rows(self._live(), _u64(r) if r.size else None,
                                          v.ctypes.data_as(ctypes.c_void_p) if v.size else None, pp, r.size),
              "szg_column_set_rows")
        del keep

    @property
    def rows(self):
        return int(self._L.szg_column_rows(self._live()))

    def info(self):
        """szg_column_get_info as a dict: kind, rows, device_bytes, and -- text columns -- heap_used and heap_capacity
        summed over the parts.  Works on a stale column."""
        out = SzgColumnInfo()
        check(self._L.szg_column_get_info(self._live(), ctypes.byref(out)), "szg_column_get_info")
        return {name: int(getattr(out, name)) for name, _ in SzgColumnInfo._fields_}

    def read(self):
        """(values, present bool[rows]) of the whole column; a text column's values are a list of bytes."""
        n = self.rows
        if self.kind == _lib.SZG_COL_STR:
            offsets = np.zeros(n + 1, dtype=np.uint64)
            w = np.zeros((n + 63) // 64, dtype=np.uint64)
            check(self._L.szg_column_read_str(self._live(), self._index._row_base, n, _u64(offsets), None, 0, None),
                  "szg_column_read_str")
            data = np.zeros(max(int(offsets[n]), 1), dtype=np.uint8)
            check(self._L.szg_column_read_str(self._live(), self._index._row_base, n, _u64(offsets), _u8(data), data.size,
                                              _u64(w) if n else None), "szg_column_read_str")
            raw = data.tobytes()
            values = [raw[int(offsets[i]):int(offsets[i + 1])] for i in range(n)]
            return values, np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)
        v = np.zeros(n, dtype=self._dtype)
        w = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(self._L.szg_column_read(self._live(), self._index._row_base, n, v.ctypes.data_as(ctypes.c_void_p) if n else None,
                                      _u64(w) if n else None), "szg_column_read")
        return v, np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)

    def _mask(self, fn, name, *args, base=None):
        if base is not None and not isinstance(base, ScanMask):
            raise TypeError("base is a ScanMask or None")
        h = ctypes.c_void_p()
        check(fn(self._live(), *args, base._live() if base is not None else None, ctypes.byref(h)), name)
        return ScanMask(self._index, h, (self._index.rows + 63) // 64)

    def where(self, op, value, base=None):
        """Rows that are present and whose value `op` the constant (op: == != < <= > >=, or SZG_CMP_*), & base.  A
        bytes / str constant is compared with a text column's values, bytewise."""
        if isinstance(value, _TEXT):
            return self._where_str(int(_CMP_OPS.get(op, op)), value, base)
        return self._mask(self._L.szg_mask_where_f64, "szg_mask_where_f64", int(_CMP_OPS.get(op, op)), float(value),
                          base=base)

    def isin(self, values, base=None):
        """Rows that are present and whose value equals one of up to 1024 constants, & base."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        return self._mask(self._L.szg_mask_where_in_f64, "szg_mask_where_in_f64", _f64(v) if v.size else None, v.size,
                          base=base)

    def codes(self, allowed, base=None):
        """U32 columns: rows that are present and whose code c has allowed[c] true (a code >= len(allowed) fails)."""
        a = np.asarray(allowed, dtype=bool).reshape(-1)
        w = pack_allow_bits(a)[0]
        return self._mask(self._L.szg_mask_where_u32, "szg_mask_where_u32", _u64(w) if w.size else None, a.size, base=base)

    def _where_str(self, op, constant, base):
        b = _text(constant)
        buf = (ctypes.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")
        return self._mask(self._L.szg_mask_where_str, "szg_mask_where_str", op, buf, len(b), base=base)

    def startswith(self, constant, base=None):
        """Text columns: rows that are present and whose value starts with the constant (at most 256 bytes), & base."""
        return self._where_str(_lib.SZG_STR_STARTS_WITH, constant, base)

    def endswith(self, constant, base=None):
        return self._where_str(_lib.SZG_STR_ENDS_WITH, constant, base)

    def contains(self, constant, base=None):
        return self._where_str(_lib.SZG_STR_CONTAINS, constant, base)

    def dfa(self, dfa, base=None):
        """Text columns: rows that are present and whose bytes -- all of them, from dfa.start -- end in an accepting
        state of the byte automaton, & base.  dfa: a regex_dfa.Dfa (regex_dfa.compile, regex_dfa.literal_set) or anything
        with its class_of / next / accept / start; the library checks the table in full before it launches."""
        class_of = np.ascontiguousarray(dfa.class_of, dtype=np.uint8).reshape(-1)
        table = np.ascontiguousarray(dfa.next, dtype=np.uint16)
        accept = np.asarray(dfa.accept, dtype=bool).reshape(-1)
        if class_of.size != 256 or table.ndim != 2 or table.shape[0] != accept.size:
            raise ValueError("a dfa has class_of[256], next[n_states, n_classes] and accept[n_states]")
        bits = pack_allow_bits(accept)[0] if accept.size else np.zeros(1, dtype=np.uint64)
        arg = _lib.SzgDfa(table.shape[0], table.shape[1], int(dfa.start), _u8(class_of),
                          table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), _u64(bits))
        return self._mask(self._L.szg_mask_where_dfa, "szg_mask_where_dfa", ctypes.byref(arg), base=base)

    def matches(self, pattern, base=None):
        """Text columns: rows that are present and in which the regular expression matches (Go's regexp.MatchString,
        the subset of regex_dfa), & base.  ValueError for a pattern outside the subset, regex_dfa.DfaTooLarge for one
        whose table exceeds the kernel's limits."""
        return self.dfa(regex_dfa.compile(pattern), base=base)

    def present(self, base=None):
        """The present rows, & base."""
        return self._mask(self._L.szg_mask_where_present, "szg_mask_where_present", base=base)

    def eq(self, value, base=None):
        return self.where("==", value, base)

    def ne(self, value, base=None):
        return self.where("!=", value, base)

    def __lt__(self, value):
        return self.where("<", value)

    def __le__(self, value):
        return self.where("<=", value)

    def __gt__(self, value):
        return self.where(">", value)

    def __ge__(self, value):
        return self.where(">=", value)


class ScanIndex:
    def __init__(self, dim, quant_bits, metric, devices=None):
        self._L = _lib.load()
        self._h = ctypes.c_void_p()
        self.dim = int(dim)
        self.quant_bits = int(quant_bits)
        self.metric = int(metric)
        dev_arr = None
        n_dev = 0
        if devices is not None:
            devices = list(devices)
            dev_arr = (ctypes.c_int * len(devices))(*devices)
            n_dev = len(devices)
        check(self._L.szg_index_create(ctypes.byref(self._h), self.dim, self.quant_bits,
                                       self.metric, dev_arr, n_dev), "szg_index_create")
        self.row_bytes = int(self._L.szg_row_bytes(self.quant_bits, self.dim))
        self._device0 = devices[0] if devices else None   # (assumed for arrays that do not name their device)
        self.options = {}   # tunables set through this object (the host mirrors consult tie_mode)
        self._comm = None
        self._masks = {}    # id -> (weak reference, handle) of every ScanMask of this handle that is still open
        self._columns = {}  # ... and of every ScanColumn
        self._row_base = 0
        # SZG_OPTIONS="name=value,...": tunables applied to every new handle (test sweeps)
        for item in os.environ.get("SZG_OPTIONS", "").split(","):
            if "=" in item:
                name, value = item.split("=", 1)
                self.set_option(name.strip(), int(value))

    # -- lifetime -----------------------------------------------------------
    def close(self):
        # columns and masks are destroyed before their handle -- also those whose Python object is already garbage
        # (its weak reference is dead, its __del__ has not run yet): their handles are destroyed here, and the entry
        # that is gone tells their close() so
        for held, destroy in (("_columns", self._L.szg_column_destroy), ("_masks", self._L.szg_mask_destroy)):
            table = getattr(self, held, {})
            for key, (ref, handle) in list(table.items()):
                m = ref()
                if m is not None:
                    m.close()
                elif table.pop(key, None) is not None:
                    destroy(ctypes.c_void_p(handle))
        if self._h:
            self._L.szg_index_destroy(self._h)
            self._h = ctypes.c_void_p()
        self._comm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- corpus ---------------------------------------------------------------
    def _rows_arg(self, rows):
        a = np.ascontiguousarray(rows, dtype=np.uint8)
        if a.size % self.row_bytes:
            raise ValueError("rows size is not a multiple of row_bytes=%d" % self.row_bytes)
        return a, a.size // self.row_bytes

    def load(self, rows):
        a, n = self._rows_arg(rows)
        check(self._L.szg_index_load(self._h, _u8(a) if n else None, n), "szg_index_load")

    def append(self, rows):
        a, n = self._rows_arg(rows)
        check(self._L.szg_index_append(self._h, _u8(a) if n else None, n), "szg_index_append")

    def append_vectors(self, vectors):
        """Bulk AddDocument from float64 vectors: quantized and packed on the device."""
        v = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, self.dim)
        check(self._L.szg_index_append_f64(self._h, _f64(v) if v.size else None, v.shape[0]),
              "szg_index_append_f64")

    def distances(self, query, rows):
        """The reference's float64 distance from `query` to each listed row."""
        q = np.ascontiguousarray(query, dtype=np.float64).reshape(-1)
        if q.size != self.dim:
            raise ValueError("query length %d != dimension %d" % (q.size, self.dim))
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        out = np.zeros(r.size, dtype=np.float64)
        check(self._L.szg_distances(self._h, _f64(q), _u64(r) if r.size else None, r.size,
                                    _f64(out) if r.size else None), "szg_distances")
        return out

    def pair_distances(self, rows_a, rows_b):
        """The reference's float64 distance between stored rows a[i] and b[i]."""
        a = np.ascontiguousarray(rows_a, dtype=np.uint64).reshape(-1)
        b = np.ascontiguousarray(rows_b, dtype=np.uint64).reshape(-1)
        if a.size != b.size:
            raise ValueError("rows_a and rows_b differ in length")
        out = np.zeros(a.size, dtype=np.float64)
        if a.size:
            check(self._L.szg_pair_distances(self._h, _u64(a), _u64(b), a.size, _f64(out)),
                  "szg_pair_distances")
        return out

    def overwrite(self, row, row_bytes):
        a, n = self._rows_arg(row_bytes)
        if n != 1:
            raise ValueError("overwrite takes exactly one row")
        check(self._L.szg_index_overwrite(self._h, int(row), _u8(a)), "szg_index_overwrite")

    def overwrite_vector(self, row, vector):
        """UpdateDocument from a float64 vector: quantized and packed on the device."""
        v = np.ascontiguousarray(vector, dtype=np.float64).reshape(-1)
        if v.size != self.dim:
            raise ValueError("vector length %d != dimension %d" % (v.size, self.dim))
        check(self._L.szg_index_overwrite_f64(self._h, int(row), _f64(v)), "szg_index_overwrite_f64")

    def tombstone(self, row):
        check(self._L.szg_index_tombstone(self._h, int(row)), "szg_index_tombstone")

    # -- bulk mutations: many rows per call, a constant number of round trips --------
    def overwrite_rows(self, rows, row_bytes):
        """overwrite() for a list: row_bytes[i] (reference encoding) replaces row rows[i].  A row out of range or listed
        twice refuses the whole call (SzgError) and nothing changes."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        a, n = self._rows_arg(row_bytes)
        if n != r.size:
            raise ValueError("%d rows of bytes for %d rows" % (n, r.size))
        check(self._L.szg_index_overwrite_rows(self._h, _u64(r) if n else None, _u8(a) if n else None, n),
              "szg_index_overwrite_rows")

    def overwrite_vectors(self, rows, vectors):
        """overwrite_vector() for a list: float64 vectors[i], quantized and packed on the device, replaces row rows[i]."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        v = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, self.dim)
        if v.shape[0] != r.size:
            raise ValueError("%d vectors for %d rows" % (v.shape[0], r.size))
        check(self._L.szg_index_overwrite_rows_f64(self._h, _u64(r) if r.size else None, _f64(v) if r.size else None, r.size),
              "szg_index_overwrite_rows_f64")

    # -- ingest from device memory: the vectors never visit the host ------------------
    def _src_rows_arg(self, src_rows):
        if src_rows is None:
            return None, None
        r = np.ascontiguousarray(src_rows, dtype=np.uint64).reshape(-1)
        return r, (_u64(r) if r.size else None)

    def append_tensor(self, t, src_rows=None):
        """append_vectors() for vectors in device memory (dev_vectors: a torch tensor or __cuda_array_interface__, in
        float64 / float32 / float16 / bfloat16, on the device of the shard that takes the rows): quantized and packed
        where they lie, the same bytes as append_vectors of the values widened to float64.  src_rows: the source row of
        each new row (any order, duplicates allowed); None appends every row of `t` in order.  The device is
        synchronised first, and `t` may be freed or rewritten once the call has returned."""
        d = dev_vectors(t, self.dim, getattr(self, "_device0", None))
        r, p = self._src_rows_arg(src_rows)
        check(self._L.szg_index_append_dev(self._h, ctypes.byref(d), p, d.n_rows if r is None else r.size),
              "szg_index_append_dev")

    def overwrite_tensor(self, rows, t, src_rows=None):
        """overwrite_vectors() for vectors in device memory (see append_tensor): source row src_rows[i] -- row i of `t`
        without a list -- replaces row rows[i].  A row out of range or listed twice refuses the whole call."""
        d = dev_vectors(t, self.dim, getattr(self, "_device0", None))
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        r, p = self._src_rows_arg(src_rows)
        if r is not None and r.size != rows.size:
            raise ValueError("%d source rows for %d rows" % (r.size, rows.size))
        check(self._L.szg_index_overwrite_rows_dev(self._h, _u64(rows) if rows.size else None, ctypes.byref(d), p, rows.size),
              "szg_index_overwrite_rows_dev")

    def tombstone_rows(self, rows):
        """tombstone() for a list (duplicates and dead rows allowed): the rows that were live and no longer are."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        dropped = ctypes.c_uint64(0)
        check(self._L.szg_index_tombstone_rows(self._h, _u64(r) if r.size else None, r.size, ctypes.byref(dropped)),
              "szg_index_tombstone_rows")
        return int(dropped.value)

    def tombstone_mask(self, mask):
        """Tombstone every live row a current ScanMask of this index allows ("delete where"); the mask stays valid.
        Returns the rows dropped."""
        if not isinstance(mask, ScanMask):
            raise TypeError("mask is a ScanMask")
        dropped = ctypes.c_uint64(0)
        check(self._L.szg_index_tombstone_mask(self._h, mask._live(), ctypes.byref(dropped)), "szg_index_tombstone_mask")
        return int(dropped.value)

    def synth(self, n_rows, seed, first_row=0):
        check(self._L.szg_index_synth(self._h, int(n_rows), int(seed), int(first_row)),
              "szg_index_synth")

    def read_rows(self, first_row, n_rows):
        out = np.zeros((int(n_rows), self.row_bytes), dtype=np.uint8)
        check(self._L.szg_index_read_rows(self._h, int(first_row), int(n_rows),
                                          _u8(out) if n_rows else None), "szg_index_read_rows")
        return out

    def fetch_into(self, t, rows=None, first_row=0, n_rows=None):
        """Stored vectors decoded into the caller's 2-D tensor in device memory (dev_vectors; float64 / float32 /
        float16 / bfloat16, on the device of the shards the rows lie on), without the host: row i of `t` receives
        stored row rows[i] -- any order, duplicates allowed, numbered as searches return them -- or, without a list,
        row first_row + i for n_rows rows (None: as many as `t` has).  The values are codec.decode_rows(read_rows(...))
        in float64, cast once to float32 for a narrower tensor and once more to float16 / bfloat16.  Columns of a wider
        tensor beside a slice and rows past the fetched ones keep what they held.  Returns `t`."""
        if hasattr(t, "data_ptr") and not getattr(t, "is_cuda", False):
            raise TypeError("a CPU tensor is host memory: read_rows() + codec.decode_rows() serve the host")
        d = dev_vectors(t, self.dim, getattr(self, "_device0", None))
        if rows is not None:
            r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
            p, n, first_row = (_u64(r) if r.size else None), r.size, 0
        else:
            p, n = None, int(d.n_rows if n_rows is None else n_rows)
        check(self._L.szg_index_fetch_rows_dev(self._h, p, int(first_row), n, ctypes.byref(d)), "szg_index_fetch_rows_dev")
        return t

    # -- compaction / reorder on the device ---------------------------------------
    def _carry_arg(self, carry):
        """carry -> (the masks, their array, the columns, their array); the arrays are None where there is nothing."""
        if isinstance(carry, (ScanMask, ScanColumn)):
            carry = [carry]
        carry = list(carry)
        for m in carry:
            if not isinstance(m, (ScanMask, ScanColumn)):
                raise TypeError("carry holds ScanMasks and ScanColumns")
        masks = [m for m in carry if isinstance(m, ScanMask)]
        columns = [c for c in carry if isinstance(c, ScanColumn)]
        marr = (ctypes.c_void_p * len(masks))(*[m._live() for m in masks]) if masks else None
        carr = (ctypes.c_void_p * len(columns))(*[c._live() for c in columns]) if columns else None
        return masks, marr, columns, carr

    def _carried(self, masks):
        words = (self.rows + 63) // 64
        for m in masks:
            m._words = words

    def reorder(self, src_rows, carry=()):
        """New row i = old row src_rows[i]; rows not listed are dropped.  The rows move on the device.  Every listed
        row must be in range, live and listed once.  carry: ScanMasks and ScanColumns of this index, in any mix.  The
        masks are rewritten for the new numbering and stay valid; the columns follow their rows on the card -- new row
        i reads what old row src_rows[i] read, a text column's heap is repacked -- and stay valid.  Every other mask
        and column becomes stale."""
        r = np.ascontiguousarray(src_rows, dtype=np.uint64).reshape(-1)
        masks, marr, columns, carr = self._carry_arg(carry)
        if columns:
            check(self._L.szg_index_reorder_carry(self._h, _u64(r) if r.size else None, r.size, marr, len(masks), carr,
                                                  len(columns)), "szg_index_reorder_carry")
        else:
            check(self._L.szg_index_reorder(self._h, _u64(r) if r.size else None, r.size, marr, len(masks)),
                  "szg_index_reorder")
        self._carried(masks)

    def compact(self, carry=()):
        """Drop the tombstoned rows on the device, keeping the order of the live ones.  Returns new_of_old,
        uint64[rows before]: the new number of each old row, 2**64 - 1 for a dropped one.  carry: as reorder's.
        Without tombstones nothing moves, and no mask or column becomes stale."""
        new_of_old = np.zeros(self.rows, dtype=np.uint64)
        masks, marr, columns, carr = self._carry_arg(carry)
        out = _u64(new_of_old) if new_of_old.size else None
        if columns:
            check(self._L.szg_index_compact_carry(self._h, out, None, marr, len(masks), carr, len(columns)),
                  "szg_index_compact_carry")
        else:
            check(self._L.szg_index_compact(self._h, out, None, marr, len(masks)), "szg_index_compact")
        self._carried(masks)
        return new_of_old

    def set_row_base(self, base):
        check(self._L.szg_index_set_row_base(self._h, int(base)), "szg_index_set_row_base")
        self._row_base = int(base)

    @property
    def rows(self):
        return int(self._L.szg_index_rows(self._h))

    @property
    def live_rows(self):
        return int(self._L.szg_index_live_rows(self._h))

    # -- search -------------------------------------------------------------
    def _allow_arg(self, allow, n_queries):
        if allow is None:
            return None, None
        a = np.asarray(allow)
        if a.dtype != np.uint64:
            a = pack_allow_bits(a)
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(n_queries, -1)
        words = (self.rows + 63) // 64
        if a.shape[1] != words:
            raise ValueError("allow mask has %d words per query, index needs %d"
                             % (a.shape[1], words))
        return a, _u64(a)

    # -- device-resident filter masks ------------------------------------------
    def mask(self, allow):
        """A ScanMask from bool[rows] or uint64 words (bit r = row r may be visited)."""
        if allow is None:
            raise ValueError("mask() needs the allowed rows")
        keep, allow_p = self._allow_arg(allow, 1)
        h = ctypes.c_void_p()
        check(self._L.szg_mask_create(self._h, allow_p, ctypes.byref(h)), "szg_mask_create")
        del keep
        return ScanMask(self, h, (self.rows + 63) // 64)

    def mask_rows(self, rows):
        """A ScanMask that allows exactly the listed rows (numbered as searches return them; duplicates allowed)."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        h = ctypes.c_void_p()
        check(self._L.szg_mask_create_rows(self._h, _u64(r) if r.size else None, r.size, ctypes.byref(h)),
              "szg_mask_create_rows")
        return ScanMask(self, h, (self.rows + 63) // 64)

    def column(self, values, present=None, kind=None):
        """A ScanColumn over the first len(values) rows.  kind: SZG_COL_F64 / SZG_COL_U32, or inferred from the dtype
        (floating -> F64, integer -> U32); present: None = every row, bool per row, or uint64 words."""
        a = np.asarray(values)
        if kind is None:
            if a.dtype.kind == "f":
                kind = _lib.SZG_COL_F64
            elif a.dtype.kind in "ui":
                kind = _lib.SZG_COL_U32
            else:
                raise ValueError("cannot infer a column kind from dtype %s" % a.dtype)
        if kind not in (_lib.SZG_COL_F64, _lib.SZG_COL_U32):
            raise ValueError("kind is SZG_COL_F64 or SZG_COL_U32")
        if kind == _lib.SZG_COL_U32 and a.dtype.kind in "ui" and a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise ValueError("codes do not fit uint32")
        v = np.ascontiguousarray(a, dtype=np.float64 if kind == _lib.SZG_COL_F64 else np.uint32).reshape(-1)
        keep, pp = ScanColumn._present_arg(present, v.size)
        h = ctypes.c_void_p()
        check(self._L.szg_column_create(self._h, kind, v.ctypes.data_as(ctypes.c_void_p) if v.size else None, pp, v.size,
                                        ctypes.byref(h)), "szg_column_create")
        del keep
        return ScanColumn(self, h, kind)

    def text_column(self, values, present=None):
        """A text ScanColumn (kind SZG_COL_STR) over the first len(values) rows: values is a sequence of bytes / str /
        None -- a str is stored as its UTF-8 bytes, None is an absent row unless `present` (as for column) says
        otherwise.  For a field whose values are mostly distinct; one with few distinct values is cheaper as codes of
        a dictionary (column, kind SZG_COL_U32)."""
        data, dp, offsets, present = _text_arg(values, present)
        keep, pp = ScanColumn._present_arg(present, offsets.size - 1)
        h = ctypes.c_void_p()
        check(self._L.szg_column_create_str(self._h, dp, _u64(offsets), pp, offsets.size - 1, ctypes.byref(h)),
              "szg_column_create_str")
        del keep, data
        return ScanColumn(self, h, _lib.SZG_COL_STR)

    def mask_stats(self):
        s = SzgMaskStats()
        check(self._L.szg_index_mask_stats(self._h, ctypes.byref(s)), "szg_index_mask_stats")
        return {name: int(getattr(s, name)) for name, _ in SzgMaskStats._fields_}

    def _masks_arg(self, masks, allow, n_queries):
        """masks= as the C array of handles: one ScanMask for every query, or a list with None entries."""
        if allow is not None:
            raise ValueError("masks= and allow= are exclusive")
        if isinstance(masks, ScanMask):
            masks = [masks]
        masks = list(masks)
        if len(masks) not in (1, n_queries):
            raise ValueError("masks= takes one ScanMask or one entry per query")
        arr = (ctypes.c_void_p * len(masks))(*[m._live() if m is not None else None for m in masks])
        return arr, len(masks)

    def search_topk(self, queries, k, allow=None, masks=None):
        """Returns (rows uint64[nq,k], dist float64[nq,k], count int32[nq]).  allow: host words or booleans per
        query; masks: one ScanMask for all queries or a list with None entries (exclusive with allow)."""
        q = np.ascontiguousarray(queries, dtype=np.float64)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.shape[1] != self.dim:
            raise ValueError("query length %d != dimension %d" % (q.shape[1], self.dim))
        nq = q.shape[0]
        k = int(k)
        out_rows = np.zeros((nq, max(k, 0)), dtype=np.uint64)
        out_dist = np.zeros((nq, max(k, 0)), dtype=np.float64)
        out_count = np.zeros(nq, dtype=np.int32)
        if masks is not None:
            arr, n_masks = self._masks_arg(masks, allow, nq)
            check(self._L.szg_search_topk_masked(self._h, _f64(q), nq, k, arr, n_masks, _u64(out_rows), _f64(out_dist),
                                                 out_count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                  "szg_search_topk_masked")
            return out_rows, out_dist, out_count
        keep, allow_p = self._allow_arg(allow, nq)
        check(self._L.szg_search_topk(self._h, _f64(q), nq, k, allow_p, _u64(out_rows),
                                      _f64(out_dist),
                                      out_count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
              "szg_search_topk")
        del keep
        return out_rows, out_dist, out_count

    def search_radius(self, query, radius, allow=None, capacity=None, masks=None):
        """Returns (rows uint64[n], dist float64[n]); grows the buffer on SZG_E_TRUNCATED."""
        q = np.ascontiguousarray(query, dtype=np.float64).reshape(-1)
        if q.size != self.dim:
            raise ValueError("query length %d != dimension %d" % (q.size, self.dim))
        if masks is not None:
            if capacity is not None:
                raise ValueError("masks= answers in full: no capacity")
            return self.search_radius_batch(q, radius, allow=allow, masks=masks)[0]
        keep, allow_p = self._allow_arg(allow, 1)
        cap = int(capacity) if capacity is not None else 1 << 16  # a too-small buffer costs a second sweep
        while True:
            out_rows = np.zeros(max(cap, 1), dtype=np.uint64)
            out_dist = np.zeros(max(cap, 1), dtype=np.float64)
            total = ctypes.c_uint64(0)
            rc = self._L.szg_search_radius(self._h, _f64(q), float(radius), allow_p,
                                           _u64(out_rows), _f64(out_dist), cap,
                                           ctypes.byref(total))
            if rc == _lib.SZG_E_TRUNCATED and capacity is None:
                cap = int(total.value)
                continue
            if rc == _lib.SZG_E_TRUNCATED:
                n = min(int(total.value), cap)
                return out_rows[:n], out_dist[:n], int(total.value)
            check(rc, "szg_search_radius")
            n = int(total.value)
            if capacity is None:
                return out_rows[:n], out_dist[:n]
            return out_rows[:n], out_dist[:n], n

    def _radius_csr(self, fn, name, queries, radii, allow, refetch=None, masks=None, capacity=None):
        q = np.ascontiguousarray(queries, dtype=np.float64)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.shape[1] != self.dim:
            raise ValueError("query length %d != dimension %d" % (q.shape[1], self.dim))
        nq = q.shape[0]
        rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float64), (nq,)))
        if masks is not None:   # (fn takes the handles and their count where the others take the words)
            filt = keep = self._masks_arg(masks, allow, nq)
        else:
            keep, allow_p = self._allow_arg(allow, nq)
            filt = (allow_p,)
        ans = self._radius_retry(lambda *out: fn(self._h, _f64(q), nq, _f64(rad), *filt, *out), name, nq, capacity, refetch)
        del keep
        return ans

    def _radius_retry(self, call, name, nq, capacity, refetch=None):
        """The batch radius calls' buffers and their grow-and-retry on SZG_E_TRUNCATED: call(out_rows, out_dist,
        capacity, out_offsets) -> the library's return code."""
        # (a truncated call is answered again from scratch: start generous, or with what the caller expects)
        cap = max(1 << 16, nq << 12) if capacity is None else max(int(capacity), 1)
        while True:
            out_rows = np.empty(max(cap, 1), dtype=np.uint64)
            out_dist = np.empty(max(cap, 1), dtype=np.float64)
            off = np.zeros(nq + 1, dtype=np.uint64)
            rc = call(_u64(out_rows), _f64(out_dist), cap, _u64(off))
            if rc == _lib.SZG_E_TRUNCATED:
                cap = int(off[nq])
                if refetch is None:
                    continue
                # a sharded call: the merged answer is kept by the communicator -- fetching it again is local (the
                # collective itself must never be repeated by some ranks only)
                out_rows = np.empty(max(cap, 1), dtype=np.uint64)
                out_dist = np.empty(max(cap, 1), dtype=np.float64)
                rc = refetch(nq, _u64(out_rows), _f64(out_dist), cap, _u64(off))
            check(rc, name)
            return [(out_rows[int(off[i]):int(off[i + 1])], out_dist[int(off[i]):int(off[i + 1])]) for i in range(nq)]

    def search_radius_batch(self, queries, radii, allow=None, masks=None, capacity=None):
        """Radius searches for a batch (radii: one value or one per query): a list of (rows, dist) per query,
        ascending distance.  The collect sweeps of the batch share query-major launches.  masks: as search_topk's.
        capacity: hits of the whole batch the first attempt has room for (default 64 Ki, or 4 Ki per query); a batch
        with more is searched a second time with room for all."""
        if masks is not None:
            return self._radius_csr(self._L.szg_search_radius_masked, "szg_search_radius_masked", queries, radii, allow,
                                    masks=masks, capacity=capacity)
        return self._radius_csr(self._L.szg_search_radius_batch, "szg_search_radius_batch", queries, radii, allow,
                                capacity=capacity)

    # -- queries from device memory: converted on the card, searched as ever ---------------
    def _queries_arg(self, t, src_rows):
        if hasattr(t, "data_ptr") and not getattr(t, "is_cuda", False):
            raise TypeError("a CPU tensor is host memory: search_topk() / search_radius_batch() take float64 on the host")
        d = dev_vectors(t, self.dim, getattr(self, "_device0", None))
        r, p = self._src_rows_arg(src_rows)
        return d, r, p, int(d.n_rows if r is None else r.size)

    def search_topk_tensor(self, t, k, src_rows=None, masks=None):
        """search_topk() for queries in device memory (dev_vectors: a 2-D torch tensor or __cuda_array_interface__ in
        float64 / float32 / float16 / bfloat16, on any device of the process): query i is row src_rows[i] of `t` (None:
        row i), widened to float64 exactly, and the answer is search_topk's for those values -- (rows, dist, count).
        masks: as search_topk's.  The tensor's device is synchronised first; `t` may be rewritten once the call returns."""
        d, r, p, nq = self._queries_arg(t, src_rows)
        k = int(k)
        out_rows = np.zeros((nq, max(k, 0)), dtype=np.uint64)
        out_dist = np.zeros((nq, max(k, 0)), dtype=np.float64)
        out_count = np.zeros(nq, dtype=np.int32)
        arr, n_masks = self._masks_arg(masks, None, nq) if masks is not None else (None, 0)
        check(self._L.szg_search_topk_dev(self._h, ctypes.byref(d), p, nq, k, arr, n_masks, _u64(out_rows), _f64(out_dist),
                                          out_count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "szg_search_topk_dev")
        return out_rows, out_dist, out_count

    def search_radius_tensor(self, t, radii, src_rows=None, masks=None, capacity=None):
        """search_radius_batch() for queries in device memory (see search_topk_tensor): a list of (rows, dist) per
        query, the same values; radii, masks and capacity as there."""
        d, r, p, nq = self._queries_arg(t, src_rows)
        rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float64), (nq,)))
        arr, n_masks = self._masks_arg(masks, None, nq) if masks is not None else (None, 0)
        return self._radius_retry(lambda *out: self._L.szg_search_radius_dev(self._h, ctypes.byref(d), p, nq, _f64(rad), arr,
                                                                              n_masks, *out),
                                  "szg_search_radius_dev", nq, capacity)

    # -- one process per GPU: the exchange inside the library (syzgydb_amd/sharded.py: Comm) ------------
    def attach_comm(self, comm):
        """Sharded searches of this handle go through `comm` (a sharded.Comm; None detaches)."""
        check(self._L.szg_index_attach_comm(self._h, comm._h if comm is not None else None), "szg_index_attach_comm")
        self._comm = comm  # keeps it alive as long as the handle uses it

    def search_topk_sharded(self, queries, k, allow=None):
        """Collective: the single-collection top-k over every rank's rows.
        Returns (rows uint64[nq,k] GLOBAL, dist float64[nq,k], count int32[nq], history_dependent bool[nq])."""
        q = np.ascontiguousarray(queries, dtype=np.float64)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.shape[1] != self.dim:
            raise ValueError("query length %d != dimension %d" % (q.shape[1], self.dim))
        nq, k = q.shape[0], int(k)
        out_rows = np.zeros((nq, max(k, 0)), dtype=np.uint64)
        out_dist = np.zeros((nq, max(k, 0)), dtype=np.float64)
        out_count = np.zeros(nq, dtype=np.int32)
        hist = np.zeros(nq, dtype=np.uint8)
        keep, allow_p = self._allow_arg(allow, nq)
        check(self._L.szg_search_topk_sharded(self._h, _f64(q), nq, k, allow_p, _u64(out_rows), _f64(out_dist),
                                              out_count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _u8(hist)),
              "szg_search_topk_sharded")
        del keep
        return out_rows, out_dist, out_count, hist.astype(bool)

    def search_radius_sharded(self, queries, radii, allow=None):
        """Collective: radius searches over every rank's rows; a list of (rows GLOBAL, dist) per query."""
        comm = self._comm
        return self._radius_csr(self._L.szg_search_radius_sharded, "szg_search_radius_sharded", queries, radii, allow,
                                refetch=lambda nq, r, d, cap, off: self._L.szg_comm_last_radius(comm._h, nq, r, d, cap, off))

    # -- diagnostics ----------------------------------------------------------
    def set_timing(self, enabled):
        """False / 0 off; True / 1 events around the scan launches; 2 also around each batch's pipeline."""
        check(self._L.szg_set_timing(self._h, int(enabled)), "szg_set_timing")

    def stats(self):
        s = SzgStats()
        check(self._L.szg_get_stats(self._h, ctypes.byref(s)), "szg_get_stats")
        return {name: getattr(s, name) for name, _ in SzgStats._fields_}

    def reset_stats(self):
        check(self._L.szg_reset_stats(self._h), "szg_reset_stats")

    def trace_certificates(self, on=True):
        """Test hook: keep what every pass hands to certification (szg_debug_trace_certificates).  Switching clears."""
        check(self._L.szg_debug_trace_certificates(self._h, int(bool(on))), "szg_debug_trace_certificates")

    def certificates(self):
        """The records of the calls made since the trace was switched on or last read, and empties the trace:
        (records, entries, dropped) -- two structured arrays with the fields of szg_cert_record (`pass` is named
        pass_) and szg_cert_entry; record r's entries are entries[r.first_entry : r.first_entry + r.n_entries].
        dropped: records that did not fit the handle's caps since the trace was switched on."""
        n_rec, n_ent, dropped = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        while True:   # (a record that another thread adds between the count and the copy: count again)
            check(self._L.szg_debug_certificates(self._h, None, 0, None, 0, ctypes.byref(n_rec), ctypes.byref(n_ent),
                                                 ctypes.byref(dropped)), "szg_debug_certificates")
            recs = np.zeros(max(1, n_rec.value), dtype=np.dtype(_lib.SzgCertRecord))
            ents = np.zeros(max(1, n_ent.value), dtype=np.dtype(_lib.SzgCertEntry))
            rc = self._L.szg_debug_certificates(self._h, recs.ctypes.data_as(ctypes.POINTER(_lib.SzgCertRecord)), recs.size,
                                                ents.ctypes.data_as(ctypes.POINTER(_lib.SzgCertEntry)), ents.size,
                                                ctypes.byref(n_rec), ctypes.byref(n_ent), ctypes.byref(dropped))
            if rc != _lib.SZG_E_TRUNCATED:
                break
        check(rc, "szg_debug_certificates")
        return recs[: n_rec.value], ents[: n_ent.value], int(dropped.value)

    def sketch_info(self):
        """Test hook: the state of the 8-bit sketch index as it stands (szg_debug_sketch_info; never a sync): a dict of
        szg_sketch_info's fields plus exc_rows, the rows without a usable sketch (uint64, ascending)."""
        info = _lib.SzgSketchInfo()
        check(self._L.szg_debug_sketch_info(self._h, ctypes.byref(info), None, 0), "szg_debug_sketch_info")
        exc = np.zeros(max(1, info.n_exc), dtype=np.uint64)
        check(self._L.szg_debug_sketch_info(self._h, ctypes.byref(info), _u64(exc), exc.size), "szg_debug_sketch_info")
        out = {name: getattr(info, name) for name, _ in _lib.SzgSketchInfo._fields_}
        out["exc_rows"] = exc[: info.n_exc]
        return out

    def sketch_masked_info(self):
        """Test hook: what the matrix sweep's masked forms (option sketch_masked) served on the sketch index since
        reset_stats (szg_debug_sketch_masked): launches that took one, skip_launches of them with the tile skip (one mask
        for every query, or tombstones alone), and the queries of all of them."""
        info = _lib.SzgSketchMaskedInfo()
        check(self._L.szg_debug_sketch_masked(self._h, ctypes.byref(info)), "szg_debug_sketch_masked")
        return {name: int(getattr(info, name)) for name, _ in _lib.SzgSketchMaskedInfo._fields_}

    def sketch_topk_stats(self):
        """What top-k searches of large k through the sketch (option sketch_topk_collect) served on the handle since
        reset_stats (szg_index_sketch_topk_stats): queries settled, fallbacks handed to the full-precision path, sample_rows
        scored (per launch), candidates gathered for the settled queries, overflows among the fallbacks."""
        s = _lib.SzgSketchTopkStats()
        check(self._L.szg_index_sketch_topk_stats(self._h, ctypes.byref(s)), "szg_index_sketch_topk_stats")
        return {name: int(getattr(s, name)) for name, _ in _lib.SzgSketchTopkStats._fields_}

    def query_prep_stats(self):
        """Which side prepared the queries of the handle's top-k calls through the sketch since reset_stats (option
        query_prep; szg_index_query_prep_stats): queries_dev, queries_host, and launches of the preparing kernel."""
        s = _lib.SzgQueryPrepStats()
        check(self._L.szg_index_query_prep_stats(self._h, ctypes.byref(s)), "szg_index_query_prep_stats")
        return {name: int(getattr(s, name)) for name, _ in _lib.SzgQueryPrepStats._fields_}

    def debug_query_prep(self, Q, on_card):
        """Test hook (szg_debug_query_prep): what a sweep of the handle's sketch would be given for the queries Q -- (images
        uint8[n, 48 * ceil(dim / 16)], constants float64[n, 5] = qnorm, m1, qscale, qconst, qnorm2) -- prepared by the host
        (on_card = 0) or by the kernel of option query_prep (1).  SzgError(SZG_E_UNSUPPORTED) on a handle without a sketch."""
        Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, self.dim)
        n = Q.shape[0]
        image = np.zeros((n, 48 * ((self.dim + 15) // 16)), dtype=np.uint8)
        meta = np.zeros((n, 5), dtype=np.float64)
        check(self._L.szg_debug_query_prep(self._h, _f64(Q), n, int(on_card), _u8(image), _f64(meta)), "szg_debug_query_prep")
        return image, meta

    @staticmethod
    def sample_plan(shard_rows, k, n_queries=1, dim=768, quant_bits=8, planes=2):
        """Host-only test hook: sample_plan() of this module."""
        return sample_plan(shard_rows, k, n_queries, dim, quant_bits, planes)

    def sketch_rows(self, first_row=0, n_rows=None):
        """Test hook: (sketch rows [first_row, first_row + n_rows) in the packed 8-bit form, uint8[n_rows, dim]; the live
        words of the sketch shards, uint64[ceil(sketch rows / 64)]) -- szg_debug_sketch_rows; never a sync."""
        total = self.sketch_info()["rows"]
        n = total - int(first_row) if n_rows is None else int(n_rows)
        out = np.zeros((n, self.dim), dtype=np.uint8)
        live = np.zeros(max(1, (total + 63) // 64), dtype=np.uint64)
        check(self._L.szg_debug_sketch_rows(self._h, int(first_row), n, _u8(out) if n else None, _u64(live), live.size),
              "szg_debug_sketch_rows")
        return out, live[: (total + 63) // 64]

    def set_option(self, name, value):
        check(self._L.szg_set_option(self._h, name.encode(), int(value)), "szg_set_option")
        self.options[name] = int(value)   # (what the host mirrors consult: e.g. tie_mode, collection.py)

    def debug_option(self, name, on_sketch=False):
        """Test hook (szg_debug_option_get): what option `name` holds on the handle, or on its internal sketch index
        (SzgError SZG_E_UNSUPPORTED while there is none; never a sync).  "contexts": the contexts in rotation."""
        out = ctypes.c_int64()
        check(self._L.szg_debug_option_get(self._h, name.encode(), int(bool(on_sketch)), ctypes.byref(out)),
              "szg_debug_option_get")
        return out.value


def f64_probe(op, a, b=None):
    """Device float64 primitive probe (tests): 0 div, 1 sqrt, 2 Go acos, 3 round, 4 f32 narrow."""
    L = _lib.load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    bb = np.ascontiguousarray(b if b is not None else a, dtype=np.float64)
    out = np.zeros_like(a)
    check(L.szg_debug_f64_probe(int(op), _f64(a), _f64(bb), _f64(out), a.size), "szg_debug_f64_probe")
    return out


def device_memory():
    """Test hook: (blocks, bytes) of device memory the library's handles, columns, masks and scratch own in this process."""
    blocks, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
    check(_lib.load().szg_debug_device_memory(ctypes.byref(blocks), ctypes.byref(nbytes)), "szg_debug_device_memory")
    return blocks.value, nbytes.value


@contextlib.contextmanager
def refuse_device_alloc(nth):
    """Test hook: inside the block, the nth device allocation from now on (nth >= 1) is refused on the host -- its call
    raises SzgError(SZG_E_NOMEM, "... (refused: test hook)").  Always disarmed on exit."""
    L = _lib.load()
    check(L.szg_debug_refuse_device_alloc(int(nth)), "szg_debug_refuse_device_alloc")
    try:
        yield
    finally:
        L.szg_debug_refuse_device_alloc(0)


def scan_group_plan(dim, quant_bits, n_queries, kp=10, scan_group=0, queries_per_launch=16, collect=False, masked=False):
    """Host-only test hook: how a one-sweep call of n_queries queries forms groups under option scan_group -- the group
    size and LDS bytes of its first launch and the passes over the rows of the whole call."""
    L = _lib.load()
    g, lds, passes = ctypes.c_int32(), ctypes.c_uint64(), ctypes.c_int32()
    check(L.szg_debug_scan_group(int(dim), int(quant_bits), int(kp), int(bool(collect)), int(bool(masked)), int(scan_group),
                                 int(n_queries), int(queries_per_launch), ctypes.byref(g), ctypes.byref(lds),
                                 ctypes.byref(passes)), "szg_debug_scan_group")
    return {"group": g.value, "lds_bytes": lds.value, "passes": passes.value}


def scan_matrix_plan(dim, quant_bits, n_queries, kp=10, planes=2, norms=True, tiled=True, masked=False, scan_group=0,
                     sketch_matrix=0):
    """Host-only test hook: whether the matrix sweep (option sketch_matrix) serves a one-sweep top-k call of n_queries
    queries -- the first launch's answer, LDS bytes and STEPS form, and the passes over the rows of the whole call."""
    L = _lib.load()
    serves, passes, lds, form = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64(), ctypes.c_int32()
    check(L.szg_debug_scan_matrix(int(dim), int(quant_bits), int(n_queries), int(kp), int(planes), int(bool(norms)),
                                  int(bool(tiled)), int(bool(masked)), int(scan_group), int(sketch_matrix),
                                  ctypes.byref(serves), ctypes.byref(passes), ctypes.byref(lds), ctypes.byref(form)),
          "szg_debug_scan_matrix")
    return {"serves": bool(serves.value), "passes": passes.value, "lds_bytes": lds.value, "steps": form.value}


def scan_select_plan(dim, quant_bits, n_queries, kp=8, planes=2, norms=True, tiled=True, masked=False, scan_group=0,
                     sketch_matrix=0, sketch_select=0):
    """Host-only test hook: which selection (option sketch_select) the first launch of a one-sweep top-k call of
    n_queries queries takes -- whether the matrix sweep serves it, and whether it then keeps row lists (lists of at most
    16 entries under sketch_select = 0) or the serial inserts."""
    L = _lib.load()
    serves, rows = ctypes.c_int32(), ctypes.c_int32()
    check(L.szg_debug_scan_select(int(dim), int(quant_bits), int(n_queries), int(kp), int(planes), int(bool(norms)),
                                  int(bool(tiled)), int(bool(masked)), int(scan_group), int(sketch_matrix),
                                  int(sketch_select), ctypes.byref(serves), ctypes.byref(rows)),
          "szg_debug_scan_select")
    return {"serves": bool(serves.value), "row_lists": bool(rows.value)}


def scan_wide_plan(dim, quant_bits, n_queries, kp=8, planes=2, norms=True, tiled=True, masked=False, scan_group=0,
                   sketch_matrix=0, sketch_select=0, sketch_wide=0):
    """Host-only test hook: the matrix sweep's two-block form (option sketch_wide) for a one-sweep top-k call of
    n_queries queries in launches of up to 32 (16 where a launch of 32 does not qualify) -- whether the form serves the
    first launch, that launch's LDS bytes, and the passes over the rows of the whole call."""
    L = _lib.load()
    serves, passes, lds = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
    check(L.szg_debug_scan_wide(int(dim), int(quant_bits), int(n_queries), int(kp), int(planes), int(bool(norms)),
                                int(bool(tiled)), int(bool(masked)), int(scan_group), int(sketch_matrix),
                                int(sketch_select), int(sketch_wide), ctypes.byref(serves), ctypes.byref(passes),
                                ctypes.byref(lds)), "szg_debug_scan_wide")
    return {"serves": bool(serves.value), "passes": passes.value, "lds_bytes": lds.value}


def scan_share_plan(dim, quant_bits, n_queries, kp=8, planes=2, norms=True, tiled=True, masked=False, scan_group=0,
                    sketch_matrix=0, sketch_select=0, sketch_wide=0, sketch_share=0):
    """Host-only test hook: the matrix sweep's shared form (option sketch_share) for a one-sweep top-k call of n_queries
    queries through the sketch -- whether a launch of min(n_queries, 64) takes it, its row slices and LDS bytes, and the
    call as it is split: the queries of its batches, its scan launches and its passes over the rows."""
    L = _lib.load()
    serves, launches, passes, slices, nb = (ctypes.c_int32() for _ in range(5))
    lds = ctypes.c_uint64()
    cap = max(1, int(n_queries))
    batches = (ctypes.c_int32 * cap)()
    check(L.szg_debug_scan_share(int(dim), int(quant_bits), int(n_queries), int(kp), int(planes), int(bool(norms)),
                                 int(bool(tiled)), int(bool(masked)), int(scan_group), int(sketch_matrix),
                                 int(sketch_select), int(sketch_wide), int(sketch_share), ctypes.byref(serves),
                                 ctypes.byref(launches), ctypes.byref(passes), ctypes.byref(slices), ctypes.byref(lds),
                                 batches, cap, ctypes.byref(nb)), "szg_debug_scan_share")
    return {"serves": bool(serves.value), "launches": launches.value, "passes": passes.value, "slices": slices.value,
            "lds_bytes": lds.value, "batches": [int(batches[i]) for i in range(min(nb.value, cap))]}


def scan_masked_plan(dim, quant_bits, n_queries, kp=8, planes=2, norms=True, tiled=True, masked=True, scan_group=0,
                     sketch_matrix=0, sketch_select=0, sketch_wide=0, sketch_share=0, sketch_masked=0, shared_mask=True):
    """Host-only test hook: the matrix sweep's masked forms (option sketch_masked) for a one-sweep top-k call of n_queries
    queries through the sketch whose launches carry masks (shared_mask: one mask for every query or tombstones alone) --
    whether a launch of min(n_queries, 64) takes a masked form, whether that is the two-block (wide) or the shared form,
    whether it skips tiles without an eligible row, its STEPS form, and the call's scan launches and passes over the rows."""
    L = _lib.load()
    p = _lib.SzgScanMaskedPlan()
    check(L.szg_debug_scan_masked(int(dim), int(quant_bits), int(n_queries), int(kp), int(planes), int(bool(norms)),
                                  int(bool(tiled)), int(bool(masked)), int(scan_group), int(sketch_matrix),
                                  int(sketch_select), int(sketch_wide), int(sketch_share), int(sketch_masked),
                                  int(bool(shared_mask)), ctypes.byref(p)), "szg_debug_scan_masked")
    out = {name: bool(getattr(p, name)) for name in ("serves", "wide", "share", "tile_skip")}
    out.update(steps=int(p.steps_form), launches=int(p.launches), passes=int(p.passes))
    return out


def scan_collect_plan(dim, quant_bits, n_queries, planes=2, norms=True, tiled=True, masked=False, scan_group=0,
                      sketch_matrix=0, sketch_wide=0):
    """Host-only test hook: the matrix sweep's collect form (radius searches through the sketch, option sketch_radius)
    for a collect call of n_queries queries with one sweep each, in launches of up to 16 (32 under sketch_wide = 2 where
    the two-block form qualifies) -- whether the form serves the first launch, whether that launch scores 32 queries per
    row read, its LDS bytes and STEPS form, and the passes over the rows of the whole call."""
    L = _lib.load()
    serves, wide, passes, lds, form = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64(), ctypes.c_int32()
    check(L.szg_debug_scan_collect(int(dim), int(quant_bits), int(n_queries), int(planes), int(bool(norms)), int(bool(tiled)),
                                   int(bool(masked)), int(scan_group), int(sketch_matrix), int(sketch_wide),
                                   ctypes.byref(serves), ctypes.byref(wide), ctypes.byref(passes), ctypes.byref(lds),
                                   ctypes.byref(form)), "szg_debug_scan_collect")
    return {"serves": bool(serves.value), "wide": bool(wide.value), "passes": passes.value, "lds_bytes": lds.value,
            "steps": form.value}


def scan_group_ring_plan(dim, quant_bits, n_queries, kp=10, scan_group=0, scan_group_ring=0):
    """Host-only test hook: the ring depth a one-sweep launch of n_queries queries takes under options scan_group and
    scan_group_ring, and the values of scan_group_ring the library accepts beside 0 (the depths it carries)."""
    L = _lib.load()
    depth, n = ctypes.c_int32(), ctypes.c_int32()
    depths = (ctypes.c_int32 * 2)()
    check(L.szg_debug_scan_group_ring(int(dim), int(quant_bits), int(kp), int(scan_group), int(n_queries),
                                      int(scan_group_ring), ctypes.byref(depth), depths, ctypes.byref(n)),
          "szg_debug_scan_group_ring")
    return {"ring_depth": depth.value, "depths": [int(depths[i]) for i in range(n.value)]}


def merge_short_plan(n_lists, m, kp):
    """Host-only test hook: whether the one-launch short-list merge serves (n_lists, m, kp) and the most entries under
    its threshold that its selection sorts (more, or a value below kp: the tournament)."""
    L = _lib.load()
    fits, sorts = ctypes.c_int32(), ctypes.c_int32()
    check(L.szg_debug_merge_short_plan(int(n_lists), int(m), int(kp), ctypes.byref(fits), ctypes.byref(sorts)),
          "szg_debug_merge_short_plan")
    return {"fits": bool(fits.value), "sorts": sorts.value}


def sample_plan(shard_rows, k, n_queries=1, dim=768, quant_bits=8, planes=2):
    """Host-only test hook (szg_debug_sample_plan): the sample plan of a top-k search through the sketch (option
    sketch_topk_collect) for one shard of shard_rows rows -- serves, stride (tiles of 16 rows), blocks (column blocks of 16
    queries per row read), tiles, sample_rows, slots (key slots per query), key_bytes, cap (entries per query the collect
    buffers start with) and lds_bytes; every field 0 where the shard is not served."""
    L = _lib.load()
    out = _lib.SzgSamplePlan()
    check(L.szg_debug_sample_plan(int(shard_rows), int(k), int(n_queries), int(dim), int(quant_bits), int(planes),
                                  ctypes.byref(out)), "szg_debug_sample_plan")
    d = {name: int(getattr(out, name)) for name, _ in _lib.SzgSamplePlan._fields_ if name != "reserved"}
    d["serves"] = bool(d["serves"])
    return d


def query_prep_serves(option, batch_queries):
    """Host-only test hook (szg_debug_query_prep_serves; csrc/sketch_plan.h): (does the card prepare a sketch top-k batch of
    batch_queries queries under query_prep = option?, the smallest batch that option 1 serves)."""
    L = _lib.load()
    least = ctypes.c_int()
    serves = L.szg_debug_query_prep_serves(int(option), int(batch_queries), ctypes.byref(least))
    return bool(serves), least.value


def option_check(name, value):
    """Host-only test hook (no device needed): raises SzgError where ScanIndex.set_option would refuse `value` for the
    one-sweep kernel's option `name` (scan_group, scan_group_ring, scan_norms, sketch_planes, sketch_matrix, sketch_select,
    sketch_wide, sketch_share, sketch_bulk, sketch_radius, sketch_masked, sketch_f64, sketch_topk_collect, query_prep)."""
    L = _lib.load()
    check(L.szg_debug_option_check(name.encode(), int(value)), "szg_debug_option_check")


KEY_FAMILIES = {"one-sweep": 0, "int8": 1, "bf16": 2, "f32": 3}


def key_eps(dim, quant_bits, metric, key, qnorm, qnorm2, family="one-sweep", planes=3, qscale=0.0, mq_qscale=0.0,
            mq_planes=0):
    """Host-only test hook (no device needed): the bound on |scan key - real-number key| that certification uses
    (csrc/key_bound.h) for the arithmetic `family` -- "one-sweep", "int8", "bf16" or "f32" (the shared sweeps).  qnorm,
    qnorm2: |g| and |g|^2 of the prepared query; qscale / mq_qscale: the integer paths' quantization steps; mq_planes: the
    digit planes of the int8 shared sweep's query (0: this build's)."""
    L = _lib.load()
    eps = ctypes.c_double()
    check(L.szg_debug_key_eps(int(dim), int(quant_bits), int(metric), int(planes), int(mq_planes), KEY_FAMILIES[family], float(key),
                              float(qnorm), float(qnorm2), float(qscale), float(mq_qscale), ctypes.byref(eps)),
          "szg_debug_key_eps")
    return eps.value


def reorder_plan(n_rows, src_rows, n_shards=1, live=None):
    """Host-only test hook (no device needed): the checks ScanIndex.reorder makes on its list -- SzgError with the same
    code and text -- and the new rows per shard.  live: bool[n_rows] (None: every row is live)."""
    L = _lib.load()
    r = np.ascontiguousarray(src_rows, dtype=np.uint64).reshape(-1)
    words = pack_allow_bits(np.asarray(live, dtype=bool))[0] if live is not None else None
    counts = np.zeros(int(n_shards), dtype=np.uint64)
    check(L.szg_debug_reorder_plan(int(n_rows), _u64(words) if words is not None and words.size else None,
                                   _u64(r) if r.size else None, r.size, int(n_shards), _u64(counts)),
          "szg_debug_reorder_plan")
    return [int(c) for c in counts]


def bulk_plan(n_rows, rows, n_shards=1, row_base=0, allow_duplicates=False):
    """Host-only test hook (no device needed): the checks the bulk mutations make on their list -- SzgError with the same
    code and text -- and its split over the shards of n_rows freshly loaded rows.  Returns one dict per shard: local
    (the shard-local rows, in the caller's order), source (the position each had in `rows`), and words, the (first,
    last) 64-row word of the shard that holds a listed row, None for a shard without one."""
    L = _lib.load()
    r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
    S = int(n_shards)
    counts, lo, hi = (np.zeros(max(S, 0), dtype=np.uint64) for _ in range(3))
    local, source = np.zeros(r.size, dtype=np.uint64), np.zeros(r.size, dtype=np.uint64)
    check(L.szg_debug_bulk_plan(int(n_rows), int(row_base), _u64(r) if r.size else None, r.size, S, int(bool(allow_duplicates)),
                                _u64(counts) if S > 0 else None, _u64(local) if r.size else None,
                                _u64(source) if r.size else None, _u64(lo) if S > 0 else None, _u64(hi) if S > 0 else None),
          "szg_debug_bulk_plan")
    out, at = [], 0
    for s in range(S):
        c = int(counts[s])
        out.append({"local": [int(x) for x in local[at:at + c]], "source": [int(x) for x in source[at:at + c]],
                    "words": (int(lo[s]), int(hi[s])) if c else None})
        at += c
    return out


def scan_plan(dim, quant_bits, n_rows, kp=10, collect=False, masked=False, cu_count=0):
    """Host-only test hook (no device needed): the lane map, launch geometry and kernel variant of a one-sweep scan
    over n_rows rows, as a dict of szg_scan_plan's fields.  Raises SzgError as szg_index_create would."""
    L = _lib.load()
    p = SzgScanPlan()
    check(L.szg_debug_scan_plan(int(dim), int(quant_bits), int(n_rows), int(kp), int(bool(collect)), int(bool(masked)),
                                int(cu_count), ctypes.byref(p)), "szg_debug_scan_plan")
    return {name: int(getattr(p, name)) for name, _ in SzgScanPlan._fields_}
