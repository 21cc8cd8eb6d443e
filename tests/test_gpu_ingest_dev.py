"""Ingest from device memory on the card (szg_index_append_dev / szg_index_overwrite_rows_dev; ScanIndex.append_tensor /
overwrite_tensor; Collection.AddDocuments with a tensor).  The device memory comes from torch tensors.  The yardstick is
the host codec on the values widened to float64 on the host, and a twin handle -- or collection -- fed those widened
values through the float64 calls; never the new code against itself.  The shapes are the smallest at which the encoder can
go wrong: a lone element, an odd nibble tail, a last piece only partly filled, the tiled (8 bits x 64, 128) and the
untiled 8-bit layout, 130 rows (past the 64-row live word and the 128-row column granule)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from syzgydb_amd import Collection, CollectionOptions, ScanIndex, SearchArgs, SzgError, SZG_COSINE, SZG_EUCLIDEAN, _lib, codec
from syzgydb_amd.index import dev_vectors, device_memory

pytestmark = pytest.mark.gpu

DEFAULT_TUNABLES = not os.environ.get("SZG_OPTIONS")
DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
BITS = (4, 8, 16, 32, 64)
DIMS = (1, 3, 33, 64, 100, 128)
N = 130
SUBNORMAL_AT = 15   # index of the smallest positive subnormal in specials()


def specials(dtype):
    """+-0, +-1, the first value past +-1, +-inf, the default quiet NaN, the largest finite value, the smallest normal
    and the smallest subnormal of `dtype` (every one exact in float64, where they are made)."""
    fi = torch.finfo(dtype)
    sub = fi.tiny * fi.eps   # 2^(emin - mantissa bits): a product of two powers of two
    vals = [0.0, -0.0, 1.0, -1.0, 1.0 + fi.eps, -1.0 - fi.eps, float("inf"), float("-inf"), float("nan"), fi.max, -fi.max,
            fi.tiny, -fi.tiny, 0.0, 0.0, sub, -sub]
    assert vals[SUBNORMAL_AT] == sub
    return torch.tensor(vals, dtype=torch.float64).to(dtype)


@functools.lru_cache(maxsize=None)
def source(name, dim, n=N, special=True, seed=0):
    """n x dim values uniform in [-1.25, 1.25] (the clamp is hit) in the source type, on the HOST; the first elements are
    specials().  Never modified."""
    g = torch.Generator().manual_seed(1000 * dim + n + seed)
    v = (torch.rand((n, dim), generator=g, dtype=torch.float64) * 2.5 - 1.25).to(DTYPES[name])
    if special:
        s = specials(DTYPES[name])
        v.view(-1)[: s.numel()] = s
    return v


def widen(t):
    return t.cpu().double().numpy()


def want_bytes(t, bits):
    with np.errstate(invalid="ignore"):   # (NaN -> integer in the host codec)
        return codec.encode_rows(widen(t), bits)


# ---- 1. bytes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", list(DTYPES))
@pytest.mark.parametrize("bits", BITS)
def test_bytes(bits, src):
    for dim in DIMS:
        t = source(src, dim).cuda()
        want = want_bytes(t, bits)
        with ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as ix, ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as twin:
            ix.append_tensor(t)
            twin.append_vectors(widen(t))
            assert ix.rows == ix.live_rows == twin.rows == N
            got = ix.read_rows(0, N)
            assert (got == want).all(), (dim, np.argwhere(got != want)[:5])
            assert (got == twin.read_rows(0, N)).all()
        if bits == 64 and src in ("f32", "bf16"):
            # flush-to-zero would show here: a float32 subnormal (bfloat16's are float32 subnormals too) reads back as
            # its exact double
            back = codec.decode_rows(got, dim, 64).reshape(-1)
            sub = float(torch.finfo(DTYPES[src]).tiny * torch.finfo(DTYPES[src]).eps)
            assert 0.0 < sub < 1.2e-38 and back[SUBNORMAL_AT] == sub and back[SUBNORMAL_AT + 1] == -sub


# ---- 2. addressing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", list(DTYPES))
def test_column_slice_of_a_wider_tensor(src):
    for bits in (4, 8, 64):
        for dim in (3, 33, 64):
            wide = source(src, dim + 5).cuda()
            t = wide[:, 2:2 + dim]   # row_stride = dim + 5, the first element two elements into the allocation
            d = dev_vectors(t, dim)
            assert d.row_stride == dim + 5 and d.data == wide.data_ptr() + 2 * wide.element_size()
            with ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as ix:
                ix.append_tensor(t)
                assert (ix.read_rows(0, N) == want_bytes(t, bits)).all(), (bits, dim)


@pytest.mark.parametrize("src", ["f16", "bf16"])
@pytest.mark.parametrize("bits", BITS)
def test_row_slice_aligned_to_the_element_only(bits, src):
    dim = 3
    flat = source(src, 1, n=N * dim + 1).cuda().view(-1)
    t = flat[1:].view(N, dim)   # starts at element 1: two bytes into the allocation, rows 6 bytes apart
    assert t.data_ptr() % 4 == 2
    with ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as ix:
        ix.append_tensor(t)
        assert (ix.read_rows(0, N) == want_bytes(t, bits)).all()


@pytest.mark.parametrize("src", list(DTYPES))
def test_source_rows_reversed_and_repeated(src):
    pick = list(range(N - 1, -1, -1)) + [5, 5, 0, N - 1, 64, 63]
    for bits, dim in ((4, 33), (8, 64), (8, 100), (16, 3), (32, 1), (64, 33)):
        t = source(src, dim).cuda()
        with ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as ix:
            ix.append_tensor(t, src_rows=pick)
            assert ix.rows == len(pick)
            assert (ix.read_rows(0, len(pick)) == want_bytes(t, bits)[pick]).all(), (bits, dim)


# ---- 3. growth and bookkeeping -----------------------------------------------------------------------------------------
def same_answers(ix, twin, Q, k=10):
    for q in (Q[:1], Q):
        r, d, c = ix.search_topk(q, k)
        r2, d2, c2 = twin.search_topk(q, k)
        assert (c == c2).all() and (r == r2).all() and (d.view(np.uint64) == d2.view(np.uint64)).all()
    radii = []
    for i in range(Q.shape[0]):   # lone queries, on both handles alike: the radius that holds the 12 nearest rows
        d, d2 = ix.search_topk(Q[i:i + 1], 12)[1][0], twin.search_topk(Q[i:i + 1], 12)[1][0]
        assert (d.view(np.uint64) == d2.view(np.uint64)).all()
        radii.append(max(float(np.sort(d2)[-1]), 1e-9))   # (dim 1 under cosine: every distance is 0 or 1; a radius is > 0)
    got, ref = ix.search_radius_batch(Q, radii), twin.search_radius_batch(Q, radii)
    for (gr, gd), (tr, td) in zip(got, ref):
        assert len(tr) >= 12 and (np.asarray(gr) == np.asarray(tr)).all()
        assert (np.asarray(gd).view(np.uint64) == np.asarray(td).view(np.uint64)).all()


@pytest.mark.parametrize("bits,dim,src,metric,options", [
    (8, 64, "bf16", SZG_COSINE, {}),
    (4, 33, "f16", SZG_EUCLIDEAN, {}),
    (16, 100, "f32", SZG_COSINE, {}),
    (32, 33, "f32", SZG_COSINE, {"sketch": 1, "sketch_min_rows": 1}),
    (64, 33, "f64", SZG_COSINE, {"sketch": 1, "sketch_min_rows": 1, "sketch_f64": 1}),
])
def test_three_appends_growth_and_searches(bits, dim, src, metric, options):
    t = source(src, dim, n=230, special=False).cuda()
    Q = widen(source("f64", dim, n=6, special=False, seed=7)) * 0.8
    with ScanIndex(dim, bits, metric, devices=[0]) as ix, ScanIndex(dim, bits, metric, devices=[0]) as twin:
        for h in (ix, twin):
            for name, value in options.items():
                h.set_option(name, value)
        at = 0
        for count in (70, 130, 30):   # 70 rows reserve 128; 200 do not fit: the second append grows the shard
            mask = ix.mask(np.ones(at, dtype=bool)) if at else None
            ix.append_tensor(t[at:at + count])
            twin.append_vectors(widen(t[at:at + count]))
            at += count
            assert ix.rows == ix.live_rows == twin.rows == at
            assert (ix.read_rows(0, at) == twin.read_rows(0, at)).all()
            same_answers(ix, twin, Q)   # (also builds the sketch the next append has to extend)
            if mask is not None:   # a mask made before the append is stale, as after append()
                with pytest.raises(SzgError) as err:
                    ix.search_topk(Q[:1], 5, masks=mask)
                assert err.value.code == _lib.SZG_E_INVALID
                mask.close()
        if options:   # the lone queries went through the sketch pre-pass, on both handles alike
            served = ix.stats()["sketch_queries"]
            print("sketch_queries", served, twin.stats()["sketch_queries"])
            assert served == twin.stats()["sketch_queries"] and (served > 0 or not DEFAULT_TUNABLES)


# ---- 4. overwrite --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,dim,src", [(8, 64, "bf16"), (8, 100, "f16"), (4, 33, "f32"), (16, 3, "f16"), (32, 1, "f64"),
                                          (64, 33, "bf16")])
def test_overwrite_two_shards(bits, dim, src):
    n = 200
    base = widen(source("f64", dim, n=n, special=False, seed=3))
    t = source(src, dim, n=80, special=False, seed=4).cuda()
    Q = widen(source("f64", dim, n=6, special=False, seed=7)) * 0.8
    rng = np.random.default_rng(bits * 1000 + dim)
    rows = rng.permutation(n)[:60].astype(np.uint64)
    rows[:6] = [199, 0, 64, 63, 128, 127]          # both shards, in mixed order
    rows = np.array(list(dict.fromkeys(rows.tolist())), dtype=np.uint64)
    pick = rng.integers(0, 80, size=rows.size)     # (duplicates among them)
    pick[:3] = [79, 0, 79]
    dead = int(rows[4])
    with ScanIndex(dim, bits, SZG_COSINE, devices=[0, 0]) as ix, ScanIndex(dim, bits, SZG_COSINE, devices=[0, 0]) as twin:
        for h in (ix, twin):
            h.load(codec.encode_rows(base, bits))
            h.search_topk(Q, 10)   # (where the width keeps row norms they exist now, and must be refreshed)
            h.tombstone(dead)
        before = ix.read_rows(0, n)
        # refusals first: nothing changes
        for bad, code in ((np.append(rows, rows[2]), _lib.SZG_E_INVALID), (np.append(rows, n), _lib.SZG_E_RANGE)):
            with pytest.raises(SzgError) as err:
                ix.overwrite_tensor(bad, t, src_rows=np.append(pick, 1))
            assert err.value.code == code
            assert ix.rows == n and ix.live_rows == n - 1 and (ix.read_rows(0, n) == before).all()
        ix.overwrite_tensor(rows, t, src_rows=pick)
        twin.overwrite_vectors(rows, widen(t)[pick])
        want = before.copy()
        want[rows.astype(np.int64)] = want_bytes(t, bits)[pick]
        got = ix.read_rows(0, n)
        assert (got == want).all() and (got == twin.read_rows(0, n)).all()
        assert ix.rows == n and ix.live_rows == twin.live_rows == n - 1   # the tombstoned row stays dead
        same_answers(ix, twin, Q)
        r, _, c = ix.search_topk(Q[:1], n)
        assert c[0] == n - 1 and dead not in set(map(int, r[0, : c[0]]))
        # without a list: entry i from source row i
        ix.overwrite_tensor(rows[:50], t)
        twin.overwrite_vectors(rows[:50], widen(t)[:50])
        assert (ix.read_rows(0, n) == twin.read_rows(0, n)).all()
        same_answers(ix, twin, Q)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    dim, bits, n = 64, 8, 10
    L = _lib.load()
    t = source("f32", dim, n=n, special=False).cuda()
    host = np.zeros((n, dim), dtype=np.float32)
    torch.cuda.empty_cache()   # (the next block comes fresh from the runtime: exactly 64 MiB, not a part of a cached one)
    big = torch.empty((1 << 24,), dtype=torch.float32, device="cuda")   # 64 MiB: torch gives it an allocation of its own
    F32 = _lib.SZG_SRC_F32
    good = dev_vectors(t, dim)

    def desc(data=good.data, dtype=F32, device=0, n_rows=n, row_stride=dim):
        return _lib.SzgDevVectors(data, dtype, device, n_rows, row_stride)

    cases = [
        ("a host buffer", desc(data=host.ctypes.data), None, n, _lib.SZG_E_INVALID, "not device memory"),
        ("row_stride < dim", desc(row_stride=dim - 1), None, n, _lib.SZG_E_INVALID, "row_stride"),
        ("an unknown dtype", desc(dtype=4), None, n, _lib.SZG_E_INVALID, "dtype"),
        ("a negative dtype", desc(dtype=-1), None, n, _lib.SZG_E_INVALID, "dtype"),
        ("data off its alignment", desc(data=good.data + 2), None, n - 1, _lib.SZG_E_INVALID, "aligned"),
        ("a source row past n_rows", desc(), [0, 1, n], 3, _lib.SZG_E_RANGE, "source row"),
        ("n_rows past src->n_rows", desc(n_rows=n - 1), None, n, _lib.SZG_E_INVALID, "n_rows"),
        ("a device ordinal out of range", desc(device=1 << 20), None, n, _lib.SZG_E_INVALID, "ordinal"),
        ("a stride that carries the last row past the allocation",
         desc(data=big.data_ptr(), n_rows=(1 << 24) // dim, row_stride=2 * dim), None, (1 << 24) // dim, _lib.SZG_E_RANGE,
         "allocation"),
        ("a listed source row past the allocation",
         desc(data=big.data_ptr(), n_rows=1 << 24, row_stride=dim), [0, (1 << 24) // dim], 2, _lib.SZG_E_RANGE, "allocation"),
    ]
    with ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as ix:
        ix.append_tensor(t)
        before = ix.read_rows(0, n)
        for what, d, src_rows, count, code, text in cases:
            r = np.asarray(src_rows, dtype=np.uint64) if src_rows is not None else None
            p = r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if r is not None else None
            rows = np.arange(min(count, n), dtype=np.uint64)
            for form in ("append", "overwrite"):
                if form == "append":
                    rc = L.szg_index_append_dev(ix._h, ctypes.byref(d), p, count)
                else:   # (the rows themselves are fine: the source is what is refused)
                    m = rows.size if r is None else min(rows.size, r.size)
                    if "stride that carries" in what:
                        continue   # (needs more entries than the handle has rows: the append form covers it)
                    rc = L.szg_index_overwrite_rows_dev(ix._h, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                        ctypes.byref(d), p, m)
                assert rc == code, (what, form, rc, L.szg_last_error())
                assert text in L.szg_last_error().decode(), (what, form, L.szg_last_error())
                assert ix.rows == ix.live_rows == n and (ix.read_rows(0, n) == before).all(), (what, form)
        # the null arguments
        assert L.szg_index_append_dev(ix._h, None, None, 1) == _lib.SZG_E_INVALID
        assert L.szg_index_overwrite_rows_dev(ix._h, None, ctypes.byref(good), None, 1) == _lib.SZG_E_INVALID
        assert L.szg_index_append_dev(ix._h, ctypes.byref(desc(data=None)), None, 1) == _lib.SZG_E_INVALID
        assert ix.rows == n and (ix.read_rows(0, n) == before).all()
        # ... and the handle still takes a good source
        ix.append_tensor(t)
        assert ix.rows == 2 * n and (ix.read_rows(n, n) == before).all()
    del big


# ---- 6. no staging for the source ------------------------------------------------------------------------------------------
def test_the_source_is_not_staged():
    dim, bits = 128, 8
    t = source("f32", dim).cuda()
    wide = widen(t)
    with ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as ix, ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as twin:
        b0 = device_memory()[1]
        ix.append_tensor(t)
        b1 = device_memory()[1]
        twin.append_vectors(wide)
        b2 = device_memory()[1]
        assert (ix.read_rows(0, N) == twin.read_rows(0, N)).all()
    grew_dev, grew_host = b1 - b0, b2 - b1
    print("device memory grew by %d bytes (append_tensor) and %d bytes (append_vectors)" % (grew_dev, grew_host))
    assert 0 < grew_dev < grew_host
    assert grew_host - grew_dev >= N * dim * 8   # the float64 staging block, which the tensor path never allocates


# ---- 7. collection -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,bits", [("f32", 8), ("bf16", 64), ("f16", 4)])
def test_collection_add_documents_with_a_tensor(src, bits):
    dim = 33
    first = widen(source("f64", dim, n=140, special=False, seed=11))
    t = source(src, dim, n=12, special=False, seed=12).cuda()
    Q = widen(source("f64", dim, n=3, special=False, seed=7)) * 0.8
    opts = dict(DistanceMethod=1, DimensionCount=dim, Quantization=bits)
    a = Collection(CollectionOptions(Name="tensor", **opts), devices=[0])
    b = Collection(CollectionOptions(Name="numpy", **opts), devices=[0])
    try:
        ids0 = list(range(100, 240))
        for c in (a, b):
            c.AddDocuments(ids0, first, [b"m%d" % i for i in ids0])
        # id 7 twice (the last entry wins), 100 / 163 / 239 exist, "1000" sorts before "9" and "7": the order is stale
        ids = [9, 100, 7, 1000, 163, 7, 50, 239, 100, 8, 20000, 3]
        metas = [b"t%d" % j for j in range(len(ids))]
        a.AddDocuments(ids, t, metas)
        b.AddDocuments(ids, widen(t), metas)
        assert a.GetAllIDs() == b.GetAllIDs() and len(a.GetAllIDs()) == 140 + 7
        assert a._order_stale == b._order_stale
        for id_ in a.GetAllIDs():
            x, y = a.GetDocument(id_), b.GetDocument(id_)
            assert (x.Vector.view(np.uint64) == y.Vector.view(np.uint64)).all() and x.Metadata == y.Metadata
        assert a.GetDocument(7).Metadata == b"t5" and a.GetDocument(100).Metadata == b"t8"
        for args in (dict(K=10), dict(Radius=0.45)):
            for v in Q:
                x, y = a.Search(SearchArgs(Vector=v, **args)), b.Search(SearchArgs(Vector=v, **args))
                assert [(r.ID, r.Distance, r.Metadata) for r in x.Results] == [(r.ID, r.Distance, r.Metadata) for r in y.Results]
                assert len(x.Results) > 0 or "K" not in args
            xs = a.SearchBatch([SearchArgs(Vector=v, **args) for v in Q])
            ys = b.SearchBatch([SearchArgs(Vector=v, **args) for v in Q])
            for x, y in zip(xs, ys):
                assert [(r.ID, r.Distance, r.Metadata) for r in x.Results] == [(r.ID, r.Distance, r.Metadata) for r in y.Results]
        with pytest.raises(ValueError, match="dimensions"):
            a.AddDocuments([1, 2], t[:2, :5], None)
    finally:
        a.Close()
        b.Close()
