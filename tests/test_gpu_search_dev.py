"""Searches whose queries lie in device memory (szg_search_topk_dev / szg_search_radius_dev; ScanIndex.search_topk_tensor /
search_radius_tensor; Collection.SearchBatchTensor).  The yardstick is the host path on the same values widened on the
host -- search_topk / search_radius_batch of t.cpu().double().numpy() -- and the comparison is exact: rows, counts, and
the float64 distances on their bits.  2 000 rows; 7 queries take a sweep per query and 40 a shared sweep under the default
options; dim 33 leaves a tail piece at every width."""
import functools

import numpy as np
import pytest
import torch

from syzgydb_amd import Collection, CollectionOptions, ScanIndex, SearchArgs, SzgError, SZG_COSINE, SZG_EUCLIDEAN, _lib, codec
from syzgydb_amd import where as W
from syzgydb_amd.index import dev_vectors

pytestmark = pytest.mark.gpu

DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
N = 2000


@functools.lru_cache(maxsize=None)
def corpus(dim, seed=0):
    v = np.random.default_rng(77 * dim + seed).random((N, dim)) * 2.0 - 1.0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def queries(dim, n, src, seed=1):
    """n x dim queries in the source type on the HOST (never modified)."""
    v = np.random.default_rng(31 * dim + n + seed).random((n, dim)) * 1.6 - 0.8
    return torch.from_numpy(v).to(DTYPES[src])


def widen(t):
    return t.cpu().double().numpy()


def index_of(bits, dim, metric):
    ix = ScanIndex(dim, bits, metric, devices=[0])
    ix.load(codec.encode_rows(corpus(dim), bits))
    return ix


def same_topk(got, want):
    (r, d, c), (r2, d2, c2) = got, want
    assert (c == c2).all(), (c, c2)
    assert (r == r2).all()
    assert (d.view(np.uint64) == d2.view(np.uint64)).all()


def same_radius(got, want):
    assert len(got) == len(want)
    for (gr, gd), (wr, wd) in zip(got, want):
        assert (np.asarray(gr) == np.asarray(wr)).all()
        assert (np.asarray(gd).view(np.uint64) == np.asarray(wd).view(np.uint64)).all()


# ---- 1. top-k ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", list(DTYPES))
@pytest.mark.parametrize("metric", [SZG_COSINE, SZG_EUCLIDEAN])
@pytest.mark.parametrize("bits", [8, 32, 64])
def test_topk(bits, metric, src):
    for dim in (96, 33):
        with index_of(bits, dim, metric) as ix:
            allow = np.random.default_rng(dim).random(N) < 0.4
            with ix.mask(allow) as some, ix.mask(~allow) as others:
                for nq in (7, 40):
                    t = queries(dim, nq, src).cuda()
                    Q = widen(t)
                    for k in (1, 10):
                        same_topk(ix.search_topk_tensor(t, k), ix.search_topk(Q, k))
                    same_topk(ix.search_topk_tensor(t, 10, masks=some), ix.search_topk(Q, 10, masks=some))
                    per_query = [(some, None, others)[i % 3] for i in range(nq)]
                    got = ix.search_topk_tensor(t, 10, masks=per_query)
                    same_topk(got, ix.search_topk(Q, 10, masks=per_query))
                    hit = set(map(int, got[0][0]))   # query 0 under `some`, query 2 under `others`
                    assert hit and all(allow[r] for r in hit) and not any(allow[int(r)] for r in got[0][2])


# ---- 2. radius ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", list(DTYPES))
@pytest.mark.parametrize("bits,metric", [(8, SZG_COSINE), (32, SZG_EUCLIDEAN), (64, SZG_COSINE), (64, SZG_EUCLIDEAN)])
def test_radius(bits, metric, src):
    dim = 33
    with index_of(bits, dim, metric) as ix:
        for nq in (7, 40):
            t = queries(dim, nq, src).cuda()
            Q = widen(t)
            d12 = ix.search_topk(Q, 12)[1]
            radii = [max(float(d12[i, 3 + i % 9]), 1e-9) for i in range(nq)]   # 4 .. 12 hits each
            radii[1] = 1e-12                                                    # ... and a query with none
            want = ix.search_radius_batch(Q, radii)
            assert len(want[1][0]) == 0 and all(len(w[0]) >= 4 for i, w in enumerate(want) if i != 1)
            same_radius(ix.search_radius_tensor(t, radii), want)
            one = float(np.median(radii))
            same_radius(ix.search_radius_tensor(t, one), ix.search_radius_batch(Q, one))
            # a first buffer far too small: truncated, grown, searched again
            total = sum(len(w[0]) for w in want)
            assert total > 3
            same_radius(ix.search_radius_tensor(t, radii, capacity=3), want)
            with ix.mask(np.arange(N) % 2 == 0) as even:
                same_radius(ix.search_radius_tensor(t, radii, masks=even), ix.search_radius_batch(Q, radii, masks=even))
                same_radius(ix.search_radius_tensor(t, radii, masks=even, capacity=1),
                            ix.search_radius_batch(Q, radii, masks=even))


def test_truncated_is_the_masked_calls_answer():
    """The C call itself: SZG_E_TRUNCATED with the offsets complete and the first `capacity` entries written, as
    szg_search_radius_masked returns it."""
    import ctypes
    dim, L = 33, _lib.load()
    u64p, f64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
    with index_of(32, dim, SZG_EUCLIDEAN) as ix:
        t = queries(dim, 5, "f32").cuda()
        Q = np.ascontiguousarray(widen(t))
        rad = np.full(5, float(ix.search_topk(Q, 6)[1].max()))
        d = dev_vectors(t, dim)
        out = []
        for fn, q in ((L.szg_search_radius_dev, None), (L.szg_search_radius_masked, Q)):
            rows, dist, off = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.float64), np.zeros(6, dtype=np.uint64)
            tail = (None, 0, rows.ctypes.data_as(u64p), dist.ctypes.data_as(f64p), 4, off.ctypes.data_as(u64p))
            if q is None:
                rc = fn(ix._h, ctypes.byref(d), None, 5, rad.ctypes.data_as(f64p), *tail)
            else:
                rc = fn(ix._h, q.ctypes.data_as(f64p), 5, rad.ctypes.data_as(f64p), *tail)
            assert rc == _lib.SZG_E_TRUNCATED
            out.append((rows, dist, off))
        assert int(out[0][2][5]) >= 30
        for a, b in zip(out[0], out[1]):
            assert (a.view(np.uint64) == b.view(np.uint64)).all()


# ---- 3. source layout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", list(DTYPES))
def test_source_rows_slices_and_element_alignment(src):
    dim, nq = 33, 12
    with index_of(8, dim, SZG_COSINE) as ix:
        t = queries(dim, nq, src).cuda()
        Q = widen(t)
        pick = list(range(nq - 1, -1, -1)) + [5, 5, 0, nq - 1]
        same_topk(ix.search_topk_tensor(t, 10, src_rows=pick), ix.search_topk(Q[pick], 10))
        same_topk(ix.search_topk_tensor(t, 3, src_rows=[4]), ix.search_topk(Q[[4]], 3))
        radii = np.linspace(0.6, 0.9, len(pick))
        same_radius(ix.search_radius_tensor(t, radii, src_rows=pick), ix.search_radius_batch(Q[pick], radii))
        # a column slice of a wider tensor
        wide = torch.zeros((nq, dim + 5), dtype=DTYPES[src], device="cuda")
        wide[:, 2:2 + dim] = t
        s = wide[:, 2:2 + dim]
        assert dev_vectors(s, dim).row_stride == dim + 5
        same_topk(ix.search_topk_tensor(s, 10), ix.search_topk(Q, 10))
        same_topk(ix.search_topk_tensor(s, 10, src_rows=pick), ix.search_topk(Q[pick], 10))
        # aligned to its element only
        flat = torch.zeros((nq * dim + 1,), dtype=DTYPES[src], device="cuda")
        flat[1:] = t.reshape(-1)
        u = flat[1:].view(nq, dim)
        assert u.data_ptr() % 16 == flat.element_size()
        same_topk(ix.search_topk_tensor(u, 10), ix.search_topk(Q, 10))
        same_radius(ix.search_radius_tensor(u, 0.8), ix.search_radius_batch(Q, 0.8))


# ---- 4. special queries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", list(DTYPES))
@pytest.mark.parametrize("bits,metric", [(8, SZG_COSINE), (32, SZG_EUCLIDEAN), (64, SZG_COSINE)])
def test_zero_and_nan_queries(bits, metric, src):
    dim = 33
    with index_of(bits, dim, metric) as ix:
        for nq in (5, 40):
            t = queries(dim, nq, src).clone()
            t[1] = 0.0
            t[3, 7] = float("nan")
            t = t.cuda()
            Q = widen(t)
            assert np.isnan(Q[3, 7]) and not Q[1].any()
            (r, d, c), (r2, d2, c2) = ix.search_topk_tensor(t, 10), ix.search_topk(Q, 10)
            assert (c == c2).all() and (r == r2).all()
            nan = np.isnan(d2)
            assert (np.isnan(d) == nan).all() and (d[~nan].view(np.uint64) == d2[~nan].view(np.uint64)).all()


@pytest.mark.parametrize("bits,dst", [(32, "f32"), (64, "f64"), (8, "f32"), (64, "bf16")])
def test_queries_that_are_fetched_rows(bits, dst):
    """ "More like this": the hits' vectors, fetched on the card, as the next queries.  Where the destination type holds
    the stored value exactly (float32 of 32-bit rows, float64 of 64-bit rows) the query coincides with its row."""
    dim = 33
    with index_of(bits, dim, SZG_EUCLIDEAN) as ix:
        for pick in ([1999, 0, 64, 777, 5], list(range(100, 140))):
            t = ix.fetch_into(torch.zeros((len(pick), dim), dtype=DTYPES[dst], device="cuda"), rows=pick)
            got = ix.search_topk_tensor(t, 5)
            same_topk(got, ix.search_topk(widen(t), 5))
            if (bits, dst) in ((32, "f32"), (64, "f64")):
                assert [int(x) for x in got[0][:, 0]] == pick and not got[1][:, 0].any()
            same_radius(ix.search_radius_tensor(t, 0.5), ix.search_radius_batch(widen(t), 0.5))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes
    dim, L = 33, _lib.load()
    with index_of(8, dim, SZG_COSINE) as ix:
        t = queries(dim, 4, "f32").cuda()
        good = dev_vectors(t, dim)
        rows, dist = np.zeros(40, dtype=np.uint64), np.zeros(40, dtype=np.float64)
        count, off, rad = np.zeros(4, dtype=np.int32), np.zeros(5, dtype=np.uint64), np.full(4, 0.5)
        u64p, f64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)

        def topk(d, src_rows=None, nq=4, k=10):
            p = src_rows.ctypes.data_as(u64p) if src_rows is not None else None
            return L.szg_search_topk_dev(ix._h, ctypes.byref(d), p, nq, k, None, 0, rows.ctypes.data_as(u64p),
                                         dist.ctypes.data_as(f64p), count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))

        def radius(d, src_rows=None, nq=4):
            p = src_rows.ctypes.data_as(u64p) if src_rows is not None else None
            return L.szg_search_radius_dev(ix._h, ctypes.byref(d), p, nq, rad.ctypes.data_as(f64p), None, 0,
                                           rows.ctypes.data_as(u64p), dist.ctypes.data_as(f64p), 40, off.ctypes.data_as(u64p))

        def desc(data=good.data, dtype=_lib.SZG_SRC_F32, device=0, n_rows=4, row_stride=dim):
            return _lib.SzgDevVectors(data, dtype, device, n_rows, row_stride)

        host = np.zeros((4, dim), dtype=np.float32)
        past = np.array([0, 4], dtype=np.uint64)
        for call in (topk, radius):
            for d, src_rows, code, text in ((desc(dtype=7), None, _lib.SZG_E_INVALID, "dtype"),
                                            (desc(row_stride=dim - 1), None, _lib.SZG_E_INVALID, "row_stride"),
                                            (desc(data=good.data + 2), None, _lib.SZG_E_INVALID, "aligned"),
                                            (desc(n_rows=3), None, _lib.SZG_E_INVALID, "n_rows"),
                                            (desc(data=host.ctypes.data), None, _lib.SZG_E_INVALID, "not device memory"),
                                            (desc(device=1 << 20), None, _lib.SZG_E_INVALID, "ordinal"),
                                            (desc(row_stride=1 << 40), None, _lib.SZG_E_RANGE, "allocation")):
                assert call(d, src_rows) == code, (text, L.szg_last_error())
                assert text in L.szg_last_error().decode()
            assert call(desc(), past, nq=2) == _lib.SZG_E_RANGE and "source row" in L.szg_last_error().decode()
        # everything else is the masked calls' refusal, after the conversion
        assert topk(desc(), k=0) == _lib.SZG_E_INVALID and "k must be > 0" in L.szg_last_error().decode()
        rad[2] = 0.0
        assert radius(desc()) == _lib.SZG_E_INVALID and "radius must be > 0" in L.szg_last_error().decode()
        with ix.mask(np.ones(N, dtype=bool)) as m:
            ix.append_vectors(corpus(dim)[:1])   # the row count moves: the mask is stale
            for call in (lambda: ix.search_topk_tensor(t, 5, masks=m), lambda: ix.search_radius_tensor(t, 0.5, masks=m)):
                with pytest.raises(SzgError, match="stale mask") as err:
                    call()
                assert err.value.code == _lib.SZG_E_INVALID
        same_topk(ix.search_topk_tensor(t, 5), ix.search_topk(widen(t), 5))   # ... and the handle still answers


# ---- 6. collection -----------------------------------------------------------------------------------------------------
def results(xs):
    return [([(r.ID, r.Distance, r.Metadata) for r in x.Results], x.PercentSearched) for x in xs]


@pytest.mark.parametrize("src,bits", [("f32", 8), ("bf16", 64), ("f16", 32)])
def test_collection_search_batch_tensor(src, bits):
    dim, n = 33, 300
    V = corpus(dim)[:n]
    c = Collection(CollectionOptions(Name="tensor", DistanceMethod=1, DimensionCount=dim, Quantization=bits), devices=[0])
    try:
        got = c.SearchBatchTensor(queries(dim, 3, src).cuda(), K=5)   # an empty collection
        assert results(got) == results(c.SearchBatch([SearchArgs(Vector=v, K=5) for v in widen(queries(dim, 3, src))]))
        assert results(got) == [([], 0.0)] * 3
        ids = list(range(100, 100 + n))
        c.AddDocuments(ids, V, [b'{"n": %d}' % i for i in ids])
        c.IndexField("n", "number")
        where = (W.Field("n") >= 150) & (W.Field("n") < 290)
        late = iter(range(1000, 2000))   # "1000" sorts before "101": an appended id leaves the order stale
        for nq in (6, 40):
            t = queries(dim, nq, src).cuda()
            Q = widen(t)
            rad = c.Search(SearchArgs(Vector=Q[0], K=8)).Results[-1].Distance   # query 0 has 8 hits within it
            assert rad > 0
            for stale in (False, True):
                for kw in (dict(K=10), dict(Radius=rad), dict(K=3, Radius=rad)):
                    for flt in (dict(), dict(Where=where), dict(Filter=lambda id_, meta: id_ % 3 == 0, FilterKey="thirds")):
                        if stale:
                            c.AddDocuments([next(late)], V[:1] * 0.5, [b'{"n": 151}'])
                            assert c._order_stale
                        got = c.SearchBatchTensor(t, **kw, **flt)
                        assert not c._order_stale   # (re-paged first, as SearchBatch does)
                        want = c.SearchBatch([SearchArgs(Vector=v, **kw, **flt) for v in Q])
                        assert results(got) == results(want), (nq, stale, kw, list(flt))
                        assert (len(got[0].Results) >= 8 or flt) and all(x.PercentSearched == 100.0 for x in got)
        with pytest.raises(ValueError, match="dimension"):
            c.SearchBatchTensor(t[:, :5], K=3)
    finally:
        c.Close()
