"""Bulk mutations on the card (szg_index_overwrite_rows / _f64, szg_index_tombstone_rows / _mask, szg_column_set_rows;
ScanIndex.overwrite_rows / overwrite_vectors / tombstone_rows / tombstone_mask, ScanColumn.set_rows; Collection.
AddDocuments / RemoveDocuments / RemoveWhere).  The yardstick throughout is a second handle -- or collection -- brought
to the same state by the single-row calls, together with the CPU oracle; never the new code against itself.  The shapes
are the smallest that cross each boundary the scatter addresses by: 16-row tiles, 64-row words and shard boundaries,
linear against tiled layout, rows that are no multiple of 16 bytes, one shard and two."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import (Collection, CollectionOptions, Field, ScanIndex, SearchArgs, SzgError, SZG_COSINE, SZG_EUCLIDEAN,
                         _lib, codec)
from syzgydb_amd.index import device_memory, refuse_device_alloc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_TUNABLES = not os.environ.get("SZG_OPTIONS")
REL_TOL = 1e-5
SEED = 0x53595A4800000000
# bits, dim: 4 x 128 and 8 x 64 are tiled; 8 x 17 is linear with a padded pitch; the others linear
LAYOUTS = [(4, 128), (8, 64), (8, 17), (16, 17), (32, 17), (64, 5)]
DEVICES = [None, [0, 0]]


@functools.lru_cache(maxsize=None)
def corpus(bits, dim, n):
    rows = orc.synth_rows(SEED + bits, 0, n, dim, bits)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def queries(dim, nq=4):
    return orc.synth_vectors(SEED + 1, 0, nq, dim)


def edge_list(n, count, seed):
    """A shuffled list of `count` distinct rows of n that holds rows 0, 15, 16, 63, 64 and n - 1."""
    edges = sorted({r for r in (0, 15, 16, 63, 64, n - 1) if r < n})
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(n), edges)
    more = rng.permutation(rest)[: max(0, count - len(edges))]
    return rng.permutation(np.concatenate([edges, more])).astype(np.uint64)


def assert_close(rows, dist, o_rows, o_dist):
    assert list(map(int, rows)) == list(map(int, o_rows)), "doc rows differ"
    d, od = np.asarray(dist, dtype=np.float64), np.asarray(o_dist, dtype=np.float64)
    assert ((np.isnan(d) & np.isnan(od)) | (np.abs(d - od) <= REL_TOL * np.abs(od))).all(), (d, od)


def check_searches(ix, rows_now, dim, bits, metric, Q, k=10, live=None, loop=None):
    """Top-k with one query and with all of Q (a shared sweep), and a radius batch, against the oracle on rows_now
    (live: bool[rows], the rows not tombstoned) -- and, where given, word for word against the loop handle."""
    allow = live.astype(np.uint8) if live is not None else None
    for q in (Q[:1], Q):
        r, d, c = ix.search_topk(q, k)
        for i in range(q.shape[0]):
            o_rows, o_dist, _ = orc.search_exact(rows_now, dim, bits, metric, q[i], k=k, allow=allow)
            assert c[i] == len(o_rows)
            assert_close(r[i, : c[i]], d[i, : c[i]], o_rows, o_dist)
        if loop is not None:
            r2, d2, c2 = loop.search_topk(q, k)
            assert (c == c2).all() and (r == r2).all() and (d.view(np.uint64) == d2.view(np.uint64)).all()
    radii = []
    for i in range(Q.shape[0]):
        dist = orc.all_distances(rows_now, dim, bits, metric, Q[i])
        radii.append(float(np.quantile(dist[live] if live is not None else dist, 0.05)))
    got = ix.search_radius_batch(Q, radii)
    for i in range(Q.shape[0]):
        o_rows, o_dist, _ = orc.search_exact(rows_now, dim, bits, metric, Q[i], radius=radii[i], allow=allow)
        assert len(o_rows) > 0
        assert_close(got[i][0], got[i][1], o_rows, o_dist)


# ---- 1. bytes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", DEVICES, ids=["one-shard", "two-shards"])
@pytest.mark.parametrize("bits,dim", LAYOUTS)
def test_overwritten_bytes(bits, dim, devices):
    for n in (17, 65, 777):
        rows = corpus(bits, dim, n)
        with ScanIndex(dim, bits, SZG_COSINE, devices=devices) as ix, ScanIndex(dim, bits, SZG_COSINE, devices=devices) as loop:
            ix.load(rows)
            loop.load(rows)
            # packed bytes
            listed = edge_list(n, max(6, n // 3), n + bits)
            fresh = orc.synth_rows(SEED + 100 + bits, 0, listed.size, dim, bits)
            want = rows.copy()
            want[listed.astype(np.int64)] = fresh
            ix.overwrite_rows(listed, fresh)
            for r, b in zip(listed, fresh):
                loop.overwrite(int(r), b)
            got = ix.read_rows(0, n)
            assert (got == loop.read_rows(0, n)).all() and (got == want).all()
            untouched = np.setdiff1d(np.arange(n), listed.astype(np.int64))
            assert (got[untouched] == rows[untouched]).all()
            # float64 vectors, encoded on the card: another list over the rows as they are now
            listed = edge_list(n, max(6, n // 2), 3 * n + bits)
            V = orc.synth_vectors(SEED + 200 + bits, 0, listed.size, dim)
            before = want.copy()
            want[listed.astype(np.int64)] = codec.encode_rows(V, bits)
            ix.overwrite_vectors(listed, V)
            for r, v in zip(listed, V):
                loop.overwrite_vector(int(r), v)
            got = ix.read_rows(0, n)
            assert (got == loop.read_rows(0, n)).all() and (got == want).all()
            untouched = np.setdiff1d(np.arange(n), listed.astype(np.int64))
            assert (got[untouched] == before[untouched]).all()
            assert ix.rows == ix.live_rows == n


# ---- 2. answers after an overwrite -----------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", DEVICES, ids=["one-shard", "two-shards"])
@pytest.mark.parametrize("metric", [SZG_COSINE, SZG_EUCLIDEAN])
@pytest.mark.parametrize("bits,dim", LAYOUTS)
def test_answers_after_overwrite(bits, dim, metric, devices):
    n = 777
    rows, Q = corpus(bits, dim, n), queries(dim)
    with ScanIndex(dim, bits, metric, devices=devices) as ix, ScanIndex(dim, bits, metric, devices=devices) as loop:
        ix.load(rows)
        loop.load(rows)
        for h in (ix, loop):   # the searches run once before: the resident norms exist and must be refreshed
            h.search_topk(Q[:1], 10)
            h.search_topk(Q, 10)
        if DEFAULT_TUNABLES:
            assert ix.stats()["mq_queries"] >= Q.shape[0]   # (the batch of four shared a sweep)
        listed = edge_list(n, 200, n + bits + metric)
        V = orc.synth_vectors(SEED + 300 + bits, 0, listed.size, dim)
        rng = np.random.default_rng(bits)
        for i in range(Q.shape[0]):   # some of the new rows become each query's nearest neighbours
            for j in range(3):
                V[4 * i + j] = np.clip(Q[i] * (1.0 - 0.1 * j) + rng.standard_normal(dim) * 0.02, -1.0, 1.0)
        now = rows.copy()
        now[listed.astype(np.int64)] = codec.encode_rows(V, bits)
        ix.overwrite_vectors(listed, V)
        for r, v in zip(listed, V):
            loop.overwrite_vector(int(r), v)
        assert (ix.read_rows(0, n) == now).all()
        check_searches(ix, now, dim, bits, metric, Q, loop=loop)
        # ... and packed bytes over rows whose norms are resident
        listed = edge_list(n, 100, 7 * n + bits + metric)
        fresh = orc.synth_rows(SEED + 400 + bits, 0, listed.size, dim, bits)
        now[listed.astype(np.int64)] = fresh
        ix.overwrite_rows(listed, fresh)
        for r, b in zip(listed, fresh):
            loop.overwrite(int(r), b)
        check_searches(ix, now, dim, bits, metric, Q, loop=loop)


# ---- 3. sketch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [100, 5000])   # 5 000 rows: more than 4 096 dirty rows, the full rebuild
def test_sketch_follows_bulk_overwrite(count):
    rng = np.random.default_rng(31 + count)
    dim, n, k = 64, 12000, 10
    V = rng.standard_normal((n, dim))
    Q = rng.standard_normal((6, dim))

    def check(ix, rows):
        for qi in range(Q.shape[0]):   # lone queries: the sketch pre-pass
            r, d, c = ix.search_topk(Q[qi], k)
            o_rows, o_dist, _ = orc.search_exact(rows, dim, 32, SZG_COSINE, Q[qi], k=k)
            assert [int(x) for x in r[0, : c[0]]] == [int(x) for x in o_rows], qi
            assert (d[0, : c[0]] == o_dist).all(), qi

    rows = orc.encode_rows(V, 32)
    with ScanIndex(dim, 32, SZG_COSINE) as ix:
        ix.load(rows)
        ix.set_option("sketch", 1)
        ix.set_option("multi_query", 0)
        check(ix, rows)
        before = ix.stats()["sketch_queries"]
        assert before > 0 or not DEFAULT_TUNABLES
        listed = rng.permutation(n)[:count].astype(np.uint64)
        W = rng.standard_normal((count, dim))
        for qi in range(Q.shape[0]):   # some of the new rows are a query's nearest neighbours
            W[2 * qi] = Q[qi] * 3.0 + rng.standard_normal(dim) * 0.01
            W[2 * qi + 1] = Q[qi] * 0.5 + rng.standard_normal(dim) * 0.05
        rows = rows.copy()
        rows[listed.astype(np.int64)] = orc.encode_rows(W, 32)
        ix.overwrite_vectors(listed, W)
        check(ix, rows)
        if DEFAULT_TUNABLES:
            assert ix.stats()["sketch_queries"] > before   # the pre-pass still answers: its sketches followed the rows
        r, _, _ = ix.search_topk(Q[0], k)
        assert int(listed[0]) in [int(x) for x in r[0]]


# ---- 4. tombstones ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", DEVICES, ids=["one-shard", "two-shards"])
@pytest.mark.parametrize("bits,dim,metric", [(8, 64, SZG_COSINE), (32, 17, SZG_EUCLIDEAN)])
def test_tombstone_rows_and_mask(bits, dim, metric, devices):
    n = 777
    rows, Q = corpus(bits, dim, n), queries(dim)
    rng = np.random.default_rng(n + bits)
    with ScanIndex(dim, bits, metric, devices=devices) as ix, ScanIndex(dim, bits, metric, devices=devices) as loop:
        ix.load(rows)
        loop.load(rows)
        live = np.ones(n, bool)

        def drop_in_loop(dead_rows):
            for r in dead_rows:
                loop.tombstone(int(r))
                live[int(r)] = False

        # the empty list and the empty mask change nothing
        older = ix.mask_rows([1, 2, 3, 500])
        assert ix.tombstone_rows([]) == 0
        with ix.mask_rows([]) as nothing:
            assert ix.tombstone_mask(nothing) == 0
        assert ix.live_rows == n
        # a list with duplicates, then one that repeats rows that are dead already
        first = np.concatenate([edge_list(n, 150, 5), [0, 64, 64, n - 1]]).astype(np.uint64)
        assert ix.tombstone_rows(first) == 150
        drop_in_loop(first)
        again = np.concatenate([first[:40], [1, 17, 448, 449]]).astype(np.uint64)
        expect = len({1, 17, 448, 449} - set(map(int, first)))
        assert ix.tombstone_rows(again) == expect
        drop_in_loop(again)
        assert ix.live_rows == loop.live_rows == int(live.sum())
        check_searches(ix, rows, dim, bits, metric, Q, live=live, loop=loop)
        # a mask from mask_rows: live and dead rows, both shards
        chosen = rng.permutation(n)[:120]
        with ix.mask_rows(chosen) as m:
            want = int(live[chosen].sum())
            assert ix.tombstone_mask(m) == want
            assert m.count == 120   # the mask itself is unchanged and still current
            assert ix.tombstone_mask(m) == 0
        drop_in_loop(chosen)
        assert ix.live_rows == loop.live_rows == int(live.sum())
        # a mask from a column comparison
        values = rng.random(n)
        with ix.column(values) as col, col.where("<", 0.2) as m:
            want = int((live & (values < 0.2)).sum())
            assert ix.tombstone_mask(m) == want
        drop_in_loop(np.flatnonzero(values < 0.2))
        assert ix.live_rows == loop.live_rows == int(live.sum())
        check_searches(ix, rows, dim, bits, metric, Q, live=live, loop=loop)
        # a mask made before all of this is still usable, in a search and as a "delete where"
        r, d, c = ix.search_topk(Q[:1], 3, masks=older)
        allow = np.zeros(n, bool)
        allow[[1, 2, 3, 500]] = True
        o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, metric, Q[0], k=3, allow=(allow & live).astype(np.uint8))
        assert_close(r[0, : c[0]], d[0, : c[0]], o_rows, o_dist)
        assert ix.tombstone_mask(older) == int((allow & live).sum())
        drop_in_loop([1, 2, 3, 500])
        older.close()
        # compact() and a search
        ix.compact()
        loop.compact()
        assert ix.rows == ix.live_rows == int(live.sum())
        assert (ix.read_rows(0, ix.rows) == rows[live]).all()
        check_searches(ix, rows[live], dim, bits, metric, Q, loop=loop)


# ---- 5. columns ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", DEVICES, ids=["one-shard", "two-shards"])
def test_column_set_rows(devices):
    n, dim = 777, 17
    rng = np.random.default_rng(n)
    with ScanIndex(dim, 8, SZG_COSINE, devices=devices) as ix:
        ix.load(corpus(8, dim, n))
        f_values, u_values = rng.random(n), rng.integers(0, 5, n).astype(np.uint32)
        f_present, u_present = rng.random(n) < 0.9, rng.random(n) < 0.9
        for values, present, new_values in ((f_values, f_present, rng.random(300) + 1.0),
                                            (u_values, u_present, rng.integers(5, 9, 300).astype(np.uint32))):
            listed = edge_list(n, 300, n + values.dtype.itemsize)
            there = rng.random(300) < 0.7
            there[:4] = [True, False, True, False]
            with ix.column(values, present=present) as col, ix.column(values, present=present) as loop:
                col.set_rows(listed, new_values, present=there)
                for r, v, t in zip(listed, new_values, there):
                    loop.set(int(r), v if t else None)
                (got_v, got_p), (want_v, want_p) = col.read(), loop.read()
                assert (got_p == want_p).all() and (got_v.view(np.uint8) == want_v.view(np.uint8)).all()
                host_v, host_p = values.copy(), present.copy()
                host_v[listed[there].astype(np.int64)] = new_values[there]
                host_p[listed.astype(np.int64)] = there
                assert (got_p == host_p).all() and (got_v[host_p] == host_v[host_p]).all()
                # masks made from the column equal the host evaluation
                if values.dtype == np.float64:
                    with col.where(">=", 1.0) as m:
                        bits = np.unpackbits(m.read().view(np.uint8), bitorder="little")[:n].astype(bool)
                    assert (bits == (host_p & (host_v >= 1.0))).all()
                else:
                    allowed = [False, True, False, True, False, True, True, False, True]
                    with col.codes(allowed) as m:
                        bits = np.unpackbits(m.read().view(np.uint8), bitorder="little")[:n].astype(bool)
                    assert (bits == (host_p & np.asarray(allowed)[host_v])).all()
                # every entry present (present=None), the empty list
                col.set_rows(listed[:5], new_values[:5])
                col.set_rows([], [])
                assert col.read()[1][listed[:5].astype(np.int64)].all()
        with ix.text_column(["a"] * n) as text:
            with pytest.raises(SzgError) as e:
                text.set_rows([0, 1], [1.0, 2.0])
            assert e.value.code == _lib.SZG_E_INVALID and "kind" in str(e.value)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", DEVICES, ids=["one-shard", "two-shards"])
def test_refusals_change_nothing(devices):
    n, dim, bits = 777, 17, 8
    rows, Q = corpus(bits, dim, n), queries(dim)
    values = np.arange(n, dtype=np.float64)
    with ScanIndex(dim, bits, SZG_COSINE, devices=devices) as ix:
        ix.load(rows)
        ix.search_topk(Q, 5)   # (norms exist)
        ix.tombstone_rows([5, 700])
        col = ix.column(values)
        fresh = orc.synth_rows(SEED + 9, 0, 3, dim, bits)
        V = orc.synth_vectors(SEED + 9, 0, 3, dim)

        def unchanged():
            assert (ix.read_rows(0, n) == rows).all() and ix.rows == n and ix.live_rows == n - 2
            v, p = col.read()
            assert (v == values).all() and p.all()

        for bad, code, text in (([3, n, 4], _lib.SZG_E_RANGE, "row out of range"),
                                ([3, 4, 2 ** 64 - 1], _lib.SZG_E_RANGE, "row out of range"),
                                ([3, 600, 3], _lib.SZG_E_INVALID, "row listed twice")):
            calls = [lambda: ix.overwrite_rows(bad, fresh), lambda: ix.overwrite_vectors(bad, V),
                     lambda: col.set_rows(bad, [1.0, 2.0, 3.0])]
            if code == _lib.SZG_E_RANGE:
                calls.append(lambda: ix.tombstone_rows(bad))
            for call in calls:
                with pytest.raises(SzgError) as e:
                    call()
                assert e.value.code == code and text in str(e.value)
                unchanged()
        # a stale mask, and one of another handle
        stale = ix.mask_rows([1, 2, 3])
        with ScanIndex(dim, bits, SZG_COSINE, devices=devices) as other:
            other.load(rows)
            foreign = other.mask_rows([1, 2, 3])
            with pytest.raises(SzgError) as e:
                ix.tombstone_mask(foreign)
            assert e.value.code == _lib.SZG_E_INVALID
            unchanged()
        ix.append(rows[:1])
        with pytest.raises(SzgError) as e:
            ix.tombstone_mask(stale)
        assert e.value.code == _lib.SZG_E_INVALID and "stale" in str(e.value)
        assert ix.live_rows == n - 1 and (ix.read_rows(0, n) == rows).all()
        col.close()


@pytest.mark.parametrize("devices", DEVICES, ids=["one-shard", "two-shards"])
def test_refused_allocation_changes_nothing(devices):
    n, dim, bits = 777, 64, 8
    rows, Q = corpus(bits, dim, n), queries(dim)
    with ScanIndex(dim, bits, SZG_COSINE, devices=devices) as ix:
        ix.load(rows)
        ix.search_topk(Q, 5)   # (norms exist)
        values = np.arange(n, dtype=np.float64)
        col = ix.column(values)
        # float64 vectors for every row need more staging than the load left behind: the call has to allocate
        listed = np.arange(n, dtype=np.uint64)[::-1].copy()
        V = orc.synth_vectors(SEED + 11, 0, n, dim)
        r0, d0, c0 = ix.search_topk(Q, 5)
        before = device_memory()
        for nth in (1, 2) if devices else (1,):
            with refuse_device_alloc(nth):
                with pytest.raises(SzgError) as e:
                    ix.overwrite_vectors(listed, V)
            assert e.value.code == _lib.SZG_E_NOMEM and "refused" in str(e.value)
            assert device_memory() == before
            assert (ix.read_rows(0, n) == rows).all() and ix.live_rows == n
            assert device_memory() == before   # (reading back fits the stage that is there)
            r1, d1, c1 = ix.search_topk(Q, 5)
            assert (r0 == r1).all() and (d0.view(np.uint64) == d1.view(np.uint64)).all()
        v, p = col.read()
        assert (v == values).all() and p.all()
        # the same call goes through once nothing is refused
        ix.overwrite_vectors(listed, V)
        assert (ix.read_rows(0, n) == codec.encode_rows(V, bits)[::-1]).all()
        col.close()


@pytest.mark.parametrize("devices", DEVICES, ids=["one-shard", "two-shards"])
def test_refused_allocation_under_set_rows_and_overwrite_rows(devices):
    """The column form and the packed-bytes form reserve their stages the same way: each has to grow the stage a load of
    5-byte rows left behind (4 096 bytes per shard), is refused, and finds everything as it was."""
    n, dim, bits = 777, 5, 8
    rows = corpus(bits, dim, n)
    values = np.arange(n, dtype=np.float64)
    listed = np.arange(n, dtype=np.uint64)[::-1].copy()
    fresh = orc.synth_rows(SEED + 12, 0, n, dim, bits)
    with ScanIndex(dim, bits, SZG_COSINE, devices=devices) as ix:
        ix.load(rows)
        ix.tombstone_rows([3, 600])
        col = ix.column(values)

        def unchanged(before):
            assert device_memory() == before
            assert (ix.read_rows(0, n) == rows).all() and ix.live_rows == n - 2
            v, p = col.read()
            assert (v == values).all() and p.all()
            assert device_memory() == before

        there = np.ones(n, bool)
        there[::5] = False
        for what, call in (("set_rows", lambda: col.set_rows(listed, values + 1000.0, present=there)),
                           ("overwrite_rows", lambda: ix.overwrite_rows(listed, fresh))):
            before = device_memory()
            for nth in (1, 2) if devices else (1,):
                with refuse_device_alloc(nth):
                    with pytest.raises(SzgError) as e:
                        call()
                assert e.value.code == _lib.SZG_E_NOMEM and "refused" in str(e.value)
                unchanged(before)
            call()   # the same call goes through once nothing is refused (and grows the stage for good)
            if what == "set_rows":
                v, p = col.read()
                assert (p == there[::-1]).all() and (v[p] == (values[::-1] + 1000.0)[p]).all()
                col.set_rows(listed, values[::-1].copy())   # back to the values and present bits `unchanged` expects
        assert (ix.read_rows(0, n) == fresh[::-1]).all() and ix.live_rows == n - 2
        col.close()


# ---- 7. collection ---------------------------------------------------------------------------------------------------
def metadata(i, tag=""):
    if i % 11 == 0:
        return b"not json"
    return ('{"price": %d, "brand": "b%d", "sku": "%ssku-%05d"}' % (i % 17, i % 5, tag, i)).encode()


def same_collections(a, b, q):
    price, brand, sku = Field("price"), Field("brand"), Field("sku")
    assert a.GetAllIDs() == b.GetAllIDs()
    for id_ in a.GetAllIDs():
        x, y = a.GetDocument(id_), b.GetDocument(id_)
        assert (x.Vector == y.Vector).all() and x.Metadata == y.Metadata
    for args in (dict(K=10), dict(K=10, Where=price < 6), dict(K=10, Where=brand == "b3"),
                 dict(K=10, Where=sku.startswith("x")), dict(K=5, Where=(price >= 3) & (brand != "b1")),
                 dict(Radius=0.45), dict(Radius=0.45, Where=price < 9)):
        for v in q:
            x, y = a.Search(SearchArgs(Vector=v, **args)), b.Search(SearchArgs(Vector=v, **args))
            assert [(r.ID, r.Distance, r.Metadata) for r in x.Results] == [(r.ID, r.Distance, r.Metadata) for r in y.Results]
            assert x.PercentSearched == y.PercentSearched
    assert len(a.Search(SearchArgs(Vector=q[0], K=10, Where=sku.startswith("x"))).Results) > 0


def test_collection_bulk_equals_loop():
    n, dim, bits = 300, 17, 8
    V = orc.synth_vectors(SEED + 20, 0, n + 100, dim)
    q = orc.synth_vectors(SEED + 21, 0, 2, dim)
    opts = dict(DistanceMethod=1, DimensionCount=dim, Quantization=bits)
    bulk = Collection(CollectionOptions(Name="bulk", **opts), devices=[0, 0])
    loop = Collection(CollectionOptions(Name="loop", **opts), devices=[0, 0])
    try:
        ids = list(range(1000, 1000 + n))
        metas = [metadata(i) for i in range(n)]
        for c in (bulk, loop):
            c.AddDocuments(ids, V[:n], metas)   # new ids only: the path both had before
            c.IndexField("price", "number")
            c.IndexField("brand", "string")
            c.IndexField("sku", "text")         # (text values go row by row)
        # a mix of existing ids, new ids and ids listed twice (an existing one, a new one)
        mix = [1000, 1015, 5000, 1063, 1064, 5001, 1015, 1299, 5000, 5002, 1127, 1011]
        mix_meta = [metadata(40 + j, "x") for j in range(len(mix))]
        mix_meta[3] = b"[1, 2]"
        bulk.AddDocuments(mix, V[n:n + len(mix)], mix_meta)
        for j, id_ in enumerate(mix):
            loop.AddDocument(id_, V[n + j], mix_meta[j])
        same_collections(bulk, loop, q)
        # RemoveDocuments: an unknown id raises before anything changes
        with pytest.raises(KeyError):
            bulk.RemoveDocuments([1001, 1002, 424242])
        same_collections(bulk, loop, q)
        gone = [1001, 1002, 1063, 1064, 5001, 1299, 1002]
        assert bulk.RemoveDocuments(gone) == 6
        for id_ in dict.fromkeys(gone):
            loop.removeDocument(id_)
        assert bulk.RemoveDocuments([]) == 0
        same_collections(bulk, loop, q)
        # RemoveWhere: through the columns, through the Filter path, and matching nothing
        price, brand = Field("price"), Field("brand")
        for expr in ((price < 3) & (brand == "b2"), Field("sku").startswith("xsku-0004"), Field("nowhere") == 1):
            victims = [id_ for id_ in loop.GetAllIDs() if expr.evaluate(loop.GetDocument(id_).Metadata)]
            assert bulk.RemoveWhere(expr) == len(victims)
            for id_ in victims:
                loop.removeDocument(id_)
            same_collections(bulk, loop, q)
        victims = [id_ for id_ in loop.GetAllIDs() if id_ % 7 == 0]
        assert len(victims) > 10 and bulk.RemoveWhere(lambda id_, meta: id_ % 7 == 0, key="sevens") == len(victims)
        for id_ in victims:
            loop.removeDocument(id_)
        same_collections(bulk, loop, q)
        assert bulk.compactions == 0
        # compaction, then removed ids that come back: the collections stay in step
        assert bulk.Compact() == loop.Compact() > 0
        same_collections(bulk, loop, q)
        back = gone[:3]
        bulk.AddDocuments(back + [1000], V[:4], [metadata(7, "x")] * 4)
        for j, id_ in enumerate(back + [1000]):
            loop.AddDocument(id_, V[j], metadata(7, "x"))
        same_collections(bulk, loop, q)
    finally:
        bulk.Close()
        loop.Close()


def test_collection_auto_compact_fires_once():
    n, dim = 200, 17
    V = orc.synth_vectors(SEED + 30, 0, n, dim)
    c = Collection(CollectionOptions(Name="auto", DistanceMethod=1, DimensionCount=dim, Quantization=8), devices=[0],
                   auto_compact=0.1)
    try:
        c.AddDocuments(range(n), V, [metadata(i) for i in range(n)])
        c.IndexField("price", "number")
        assert c.RemoveDocuments(range(10)) == 10 and c.compactions == 0       # 5 % dead: below the rule
        assert c.RemoveDocuments(range(10, 70)) == 60 and c.compactions == 1   # 35 %: one compaction, not sixty
        assert c._index.rows == c._index.live_rows == n - 70
        assert c.RemoveWhere(Field("price") < 4) > 13 and c.compactions == 2
        assert c._index.rows == c._index.live_rows == len(c.GetAllIDs())
        res = c.Search(SearchArgs(Vector=V[100], K=1))
        assert res.Results[0].ID == 100 and res.Results[0].Metadata == metadata(100)
    finally:
        c.Close()


def test_cpp_bulk_collection_mirror(tmp_path):
    exe = tmp_path / "test_bulk_collection"
    lib_dir = os.path.join(ROOT, "syzgydb_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_bulk_collection.cpp"), "-o", str(exe),
                           "-L", lib_dir, "-lsyzgy_scan", "-Wl,-rpath," + lib_dir])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "CPP_BULK_OK" in p.stdout
