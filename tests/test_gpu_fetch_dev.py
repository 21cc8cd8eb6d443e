"""Stored vectors decoded into device memory on the card (szg_index_fetch_rows_dev; ScanIndex.fetch_into;
Collection.FetchVectors).  The yardstick is the host route the call replaces, never the new code against itself:
codec.decode_rows(index.read_rows(...)) gives the float64 values; a float32 destination holds them cast once
(round-to-nearest-even), a float16 / bfloat16 destination that float32 cast once more -- `.double().float().half()` on a
CPU tensor -- and the comparison is on the bits, NaNs equal.  The shapes are the smallest at which the decoder can go wrong:
a lone element, an odd nibble tail, a last piece only partly filled (33), whole 64-byte steps (64, 192: the tiled layout at
8 bits), neither (100), 300 rows (more than one block at every width)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from syzgydb_amd import Collection, CollectionOptions, ScanIndex, SzgError, SZG_COSINE, _lib, codec
from syzgydb_amd.index import dev_vectors, device_memory

pytestmark = pytest.mark.gpu

DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
INTS = {torch.float64: torch.int64, torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
BITS = (4, 8, 16, 32, 64)
DIMS = (1, 3, 33, 64, 100, 192)
N = 300
SENTINEL = 7.0   # exact in all four types; no stored value below is 7


@functools.lru_cache(maxsize=None)
def vectors(dim, n=N, seed=0):
    """n x dim float64 uniform in [-1.25, 1.25] (the clamp of the narrow widths is hit), on the host.  Never modified."""
    v = np.random.default_rng(1000 * dim + n + seed).random((n, dim)) * 2.5 - 1.25
    v.setflags(write=False)
    return v


def chain(f64, dtype):
    """The rule of the header on the CPU: float64 -> (one cast) float32 -> (one more) float16 / bfloat16."""
    t = torch.from_numpy(np.array(f64, dtype=np.float64))   # (a copy: the cached inputs are read-only)
    if dtype == torch.float64:
        return t
    t = t.float()
    return t if dtype == torch.float32 else t.to(dtype)


def stored(ix, dtype, first=0, n=None):
    """What rows [first, first + n) hold, through the host route, in `dtype` on the CPU."""
    n = ix.rows - first if n is None else n
    return chain(codec.decode_rows(ix.read_rows(first, n), ix.dim, ix.quant_bits), dtype)


def same_bits(got, want):
    """got (any device) == want (CPU) on the bits, NaNs equal."""
    got = got.detach().cpu().contiguous()
    want = want.contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        return False
    iv = INTS[want.dtype]
    return torch.equal(got.view(iv)[~nan], want.view(iv)[~nan])


def empty(n, dim, dtype):
    return torch.full((n, dim), SENTINEL, dtype=dtype, device="cuda")


def index_of(bits, dim, n=N, devices=(0,), seed=0):
    ix = ScanIndex(dim, bits, SZG_COSINE, devices=list(devices))
    ix.load(codec.encode_rows(vectors(dim, n, seed), bits))
    return ix


# ---- 1. values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", list(DTYPES))
@pytest.mark.parametrize("bits", BITS)
def test_values(bits, dst):
    dtype = DTYPES[dst]
    for dim in DIMS:
        with index_of(bits, dim) as ix:
            out = empty(N, dim, dtype)   # a fresh block: 16-byte aligned, so dims whose rows are whole 16 bytes take
            assert out.data_ptr() % 16 == 0   # the vector store form, the others the element-wise one
            assert ix.fetch_into(out) is out
            want = stored(ix, dtype)
            assert not torch.isnan(want).any()
            assert torch.equal(out.cpu().view(INTS[dtype]), want.view(INTS[dtype])), (bits, dst, dim)


def test_the_vector_store_form_and_the_element_form_agree_with_the_host():
    """dim 64: every row of every type is a multiple of 16 bytes and the block is aligned (vector stores); the same rows
    into a destination one element further on (f16 / bf16 / f32: aligned to the element only) take element stores."""
    dim = 64
    for bits in BITS:
        with index_of(bits, dim) as ix:
            for dtype in (torch.float32, torch.float16, torch.bfloat16):
                flat = torch.full((N * dim + 1,), SENTINEL, dtype=dtype, device="cuda")
                out = flat[1:].view(N, dim)
                assert out.data_ptr() % 16 == flat.element_size() and flat.data_ptr() % 16 == 0
                ix.fetch_into(out)
                want = stored(ix, dtype)
                assert same_bits(out, want), (bits, dtype)
                assert float(flat[0]) == SENTINEL
                aligned = empty(N, dim, dtype)
                ix.fetch_into(aligned)
                assert same_bits(aligned, want), (bits, dtype)


@pytest.mark.parametrize("dst", list(DTYPES))
def test_non_finite_values_overflow_and_subnormals(dst):
    dtype = DTYPES[dst]
    dim = 9
    sub32 = float(np.float32(2.0 ** -149))
    v = vectors(dim, 4).copy()
    v[0, :7] = [np.nan, np.inf, -np.inf, sub32, -sub32, 0.0, -0.0]
    v[1, :6] = [1e39, -1e39, 70000.0, -70000.0, 65520.0, 3.0e-8]   # inf in float32; inf in float16; a tie that rounds up
    v[2, :3] = [1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -40, 1.0 + 2.0 ** -9]   # ties and double rounding on the way down
    for bits in (32, 64):
        with ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as ix:
            with np.errstate(over="ignore"):
                ix.load(codec.encode_rows(v, bits))
            out = empty(4, dim, dtype)
            ix.fetch_into(out)
            want = stored(ix, dtype)
            assert torch.isnan(want[0, 0]) and torch.isinf(want[0, 1])
            if bits == 64 and dtype != torch.float64:
                assert torch.isinf(want[1, 0]) and want[1, 0] > 0 and torch.isinf(want[1, 1]) and want[1, 1] < 0
            if dtype == torch.float16:
                assert torch.isinf(want[1, 2]) and torch.isinf(want[1, 3]) and want[1, 3] < 0
            if dtype in (torch.float32, torch.float64):   # (flush-to-zero would show here)
                assert float(want[0, 3]) == sub32 and float(out[0, 3]) == sub32
            assert same_bits(out, want), (bits, dst, out.cpu(), want)


# ---- 2. which rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,dim,dst", [(4, 33, "f16"), (8, 64, "bf16"), (8, 100, "f32"), (16, 3, "f64"), (32, 192, "f32"),
                                          (64, 33, "f16")])
def test_listed_rows_and_ranges(bits, dim, dst):
    dtype = DTYPES[dst]
    with index_of(bits, dim) as ix:
        all_rows = stored(ix, dtype)
        for pick in (list(range(N - 1, -1, -1)), [5, 5, 0, N - 1, 64, 63, 5, 16, 15], [N - 1], [0]):
            out = empty(len(pick), dim, dtype)
            ix.fetch_into(out, rows=pick)
            assert same_bits(out, all_rows[pick]), (pick[:4],)
        for first, n in ((17, N - 17), (N - 1, 1), (1, 40), (0, N)):
            out = empty(n, dim, dtype)
            ix.fetch_into(out, first_row=first, n_rows=n)
            assert same_bits(out, all_rows[first:first + n]), (first, n)
        ix.fetch_into(empty(0, dim, dtype))   # nothing asked, nothing done
        ix.fetch_into(empty(4, dim, dtype), rows=[])


# ---- 3. destination layout ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", list(DTYPES))
def test_column_slice_and_spare_rows_keep_their_sentinel(dst):
    dtype = DTYPES[dst]
    for bits, dim in ((4, 33), (8, 64), (32, 3), (64, 100)):
        with index_of(bits, dim) as ix:
            n = N - 10
            wide = empty(N + 6, dim + 5, dtype)
            out = wide[:, 2:2 + dim]   # row_stride = dim + 5, the first element two elements into the block
            d = dev_vectors(out, dim)
            assert d.row_stride == dim + 5 and d.data == wide.data_ptr() + 2 * wide.element_size()
            ix.fetch_into(out, first_row=3, n_rows=n)
            got = wide.cpu()
            assert same_bits(got[:n, 2:2 + dim], stored(ix, dtype, 3, n)), (bits, dim)
            got[:n, 2:2 + dim] = SENTINEL
            assert bool((got == SENTINEL).all()), (bits, dim)   # every element outside [0, n) x [0, dim) is untouched
            # ... and with a list
            wide.fill_(SENTINEL)
            pick = [N - 1, 0, 7, 7]
            ix.fetch_into(out, rows=pick)
            got = wide.cpu()
            assert same_bits(got[:4, 2:2 + dim], stored(ix, dtype)[pick])
            got[:4, 2:2 + dim] = SENTINEL
            assert bool((got == SENTINEL).all())


@pytest.mark.parametrize("dst", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("bits", BITS)
def test_destination_aligned_to_its_element_only(bits, dst):
    dtype = DTYPES[dst]
    dim = 3
    flat = torch.full((N * dim + 2,), SENTINEL, dtype=dtype, device="cuda")
    out = flat[1:1 + N * dim].view(N, dim)   # starts one element into the block: rows 3 elements apart
    assert out.data_ptr() % 16 == flat.element_size()
    with index_of(bits, dim) as ix:
        ix.fetch_into(out)
        assert same_bits(out, stored(ix, dtype))
    assert float(flat[0]) == SENTINEL and float(flat[-1]) == SENTINEL


# ---- 4. state of the handle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,dim,dst", [(8, 64, "bf16"), (4, 33, "f32"), (32, 100, "f16"), (64, 3, "f64")])
def test_two_shards_on_one_card(bits, dim, dst):
    dtype = DTYPES[dst]
    with index_of(bits, dim, devices=(0, 0)) as ix:
        all_rows = stored(ix, dtype)
        half = N // 2
        pick = [N - 1, 0, half, half - 1, half + 1, 3, N - 2, half, 0] + list(range(100, 220))[::-1]
        out = empty(len(pick), dim, dtype)
        ix.fetch_into(out, rows=pick)
        assert same_bits(out, all_rows[pick])
        out = empty(60, dim, dtype)
        ix.fetch_into(out, first_row=half - 30, n_rows=60)   # a range across the boundary
        assert same_bits(out, all_rows[half - 30:half + 30])
        out = empty(N, dim, dtype)
        ix.fetch_into(out)
        assert same_bits(out, all_rows)


def test_tombstones_overwrites_and_a_row_base():
    dim, bits, dtype = 33, 8, torch.float32
    with index_of(bits, dim) as ix:
        before = stored(ix, dtype)
        dead = [0, 5, 64, N - 1]
        ix.tombstone_rows(dead)
        out = empty(N, dim, dtype)
        ix.fetch_into(out)
        assert ix.live_rows == N - len(dead) and same_bits(out, before)   # dead rows are served as stored
        fresh = torch.from_numpy(vectors(dim, 6, seed=9).copy()).to(torch.bfloat16).cuda()
        rows = [7, 1, 5, 200, 63, N - 2]
        ix.overwrite_tensor(rows, fresh)
        after = stored(ix, dtype)
        assert not torch.equal(after[rows], before[rows])
        out = empty(len(rows), dim, dtype)
        ix.fetch_into(out, rows=rows)
        assert same_bits(out, after[rows])
        assert same_bits(out, chain(codec.decode_rows(codec.encode_rows(fresh.cpu().double().numpy(), bits), dim, bits), dtype))
        # rows are numbered as searches return them
        base = 1 << 33
        ix.set_row_base(base)
        q = codec.decode_rows(ix.read_rows(9, 1), dim, bits)
        hit = int(ix.search_topk(q, 1)[0][0, 0])
        assert hit >= base
        out = empty(3, dim, dtype)
        ix.fetch_into(out, rows=[hit, base, base + N - 1])
        assert same_bits(out, after[[hit - base, 0, N - 1]])
        ix.fetch_into(out, first_row=base + 10, n_rows=3)
        assert same_bits(out, after[10:13])
        for kw in (dict(rows=[9]), dict(rows=[base + N]), dict(first_row=9, n_rows=1), dict(first_row=base + N - 1, n_rows=2)):
            with pytest.raises(SzgError) as err:
                ix.fetch_into(out, **kw)
            assert err.value.code == _lib.SZG_E_RANGE, kw


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    dim, bits, n = 64, 8, 10
    L = _lib.load()
    host = np.zeros((n, dim), dtype=np.float32)
    torch.cuda.empty_cache()   # (the next block comes fresh from the runtime: exactly 64 MiB, not a part of a cached one)
    big = torch.full((1 << 24,), SENTINEL, dtype=torch.float32, device="cuda")   # 64 MiB: an allocation of its own
    out = empty(n, dim, torch.float32)
    good = dev_vectors(out, dim)
    F32 = _lib.SZG_SRC_F32

    def desc(data=good.data, dtype=F32, device=0, n_rows=n, row_stride=dim):
        return _lib.SzgDevVectors(data, dtype, device, n_rows, row_stride)

    def u64(a):
        return np.asarray(a, dtype=np.uint64)

    with index_of(bits, dim, n=80) as ix:
        rows_n = ix.rows
        cases = [
            ("a host buffer", desc(data=host.ctypes.data), None, 0, n, _lib.SZG_E_INVALID, "not device memory"),
            ("row_stride < dim", desc(row_stride=dim - 1), None, 0, n, _lib.SZG_E_INVALID, "row_stride"),
            ("an unknown dtype", desc(dtype=4), None, 0, n, _lib.SZG_E_INVALID, "dtype"),
            ("a negative dtype", desc(dtype=-1), None, 0, n, _lib.SZG_E_INVALID, "dtype"),
            ("data off its alignment", desc(data=good.data + 2), None, 0, n - 1, _lib.SZG_E_INVALID, "aligned"),
            ("n_rows past dst->n_rows", desc(n_rows=n - 1), None, 0, n, _lib.SZG_E_INVALID, "n_rows"),
            ("a list longer than dst->n_rows", desc(n_rows=2), u64([0, 1, 2]), 0, 3, _lib.SZG_E_INVALID, "n_rows"),
            ("a device ordinal out of range", desc(device=1 << 20), None, 0, n, _lib.SZG_E_INVALID, "ordinal"),
            ("a null data pointer", desc(data=None), None, 0, 1, _lib.SZG_E_INVALID, "null argument"),
            ("a stride that carries the last row past the allocation",
             desc(data=big.data_ptr(), n_rows=rows_n, row_stride=(1 << 24) // (rows_n - 1) + 1), None, 0, rows_n, _lib.SZG_E_RANGE,
             "allocation"),
            ("a listed row past the handle", desc(), u64([0, rows_n]), 0, 2, _lib.SZG_E_RANGE, "row out of range"),
            ("a range past the handle", desc(), None, rows_n - n + 1, n, _lib.SZG_E_RANGE, "row range"),
            ("a first row past the handle", desc(), None, rows_n + 1, 1, _lib.SZG_E_RANGE, "row range"),
        ]
        for what, d, rows, first, count, code, text in cases:
            p = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if rows is not None else None
            rc = L.szg_index_fetch_rows_dev(ix._h, p, first, count, ctypes.byref(d))
            assert rc == code, (what, rc, L.szg_last_error())
            assert text in L.szg_last_error().decode(), (what, L.szg_last_error())
            assert bool((out == SENTINEL).all()), what
        assert bool((big == SENTINEL).all())
        assert L.szg_index_fetch_rows_dev(ix._h, None, 0, 1, None) == _lib.SZG_E_INVALID
        # n_rows == 0 checks the descriptor only: a bad one is refused, a good one passes whatever the rows say
        assert L.szg_index_fetch_rows_dev(ix._h, None, 0, 0, ctypes.byref(desc(dtype=9))) == _lib.SZG_E_INVALID
        assert L.szg_index_fetch_rows_dev(ix._h, None, 0, 0, ctypes.byref(desc(row_stride=1))) == _lib.SZG_E_INVALID
        assert L.szg_index_fetch_rows_dev(ix._h, None, 1 << 40, 0, ctypes.byref(desc(data=None, n_rows=0))) == _lib.SZG_OK
        assert bool((out == SENTINEL).all())
        # ... and the handle still serves a good destination
        ix.fetch_into(out, first_row=rows_n - n, n_rows=n)
        assert same_bits(out, stored(ix, torch.float32, rows_n - n, n))
    del big


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second card")
def test_a_destination_on_another_device_is_refused():
    dim = 8
    with index_of(8, dim, n=20) as ix:
        out = torch.full((20, dim), SENTINEL, dtype=torch.float32, device="cuda:1")
        with pytest.raises(SzgError, match="destination on another device") as err:
            ix.fetch_into(out)
        assert err.value.code == _lib.SZG_E_INVALID and bool((out == SENTINEL).all())


# ---- 6. nothing but the list is staged ---------------------------------------------------------------------------------
def test_only_the_list_is_staged():
    dim, bits, n = 128, 8, 600
    src = torch.from_numpy(vectors(dim, n).copy()).float().cuda()
    out = empty(n, dim, torch.float32)
    with ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as ix:
        ix.append_tensor(src)   # (read in place: the handle has staged nothing so far)
        b0 = device_memory()[1]
        ix.fetch_into(out)
        b1 = device_memory()[1]
        pick = np.random.default_rng(1).integers(0, n, size=n)
        ix.fetch_into(out, rows=pick)
        b2 = device_memory()[1]
        ix.fetch_into(out, rows=pick[::-1].copy())
        b3 = device_memory()[1]
        assert same_bits(out, stored(ix, torch.float32)[pick[::-1].copy()])
    print("library device bytes grew by %d (a range), %d (a list of %d rows), %d (a second list)" % (b1 - b0, b2 - b1, n, b3 - b2))
    assert b1 == b0            # a range stages nothing
    assert 0 < b2 - b1 <= 8 * n   # a list: 8 bytes per row, nothing for the rows or the values (n * dim * 4 bytes)
    assert b3 == b2


# ---- 7. collection -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,dst", [(8, "f32"), (64, "f64"), (4, "bf16")])
def test_collection_fetch_vectors(bits, dst):
    dim, dtype = 33, DTYPES[dst]
    V = vectors(dim, 140, seed=11)
    c = Collection(CollectionOptions(Name="fetch", DistanceMethod=1, DimensionCount=dim, Quantization=bits), devices=[0])
    try:
        ids = list(range(100, 240))
        c.AddDocuments(ids, V, [b"m%d" % i for i in ids])
        for gone in (100, 163, 164, 239):
            c.removeDocument(gone)
        c.Compact()
        ask = [238, 101, 165, 162, 101, 200]
        out = empty(len(ask), dim, dtype)
        assert c.FetchVectors(ask, out) is out
        want = chain(np.stack([c.GetDocument(i).Vector for i in ask]), dtype)
        assert same_bits(out, want)
        assert same_bits(out, chain(codec.decode_rows(codec.encode_rows(V[[i - 100 for i in ask]], bits), dim, bits), dtype))
        out.fill_(SENTINEL)
        with pytest.raises(KeyError, match="record not found"):
            c.FetchVectors([238, 163, 101], out)   # 163 was removed
        assert bool((out == SENTINEL).all())
    finally:
        c.Close()
