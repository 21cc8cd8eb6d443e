"""Device-resident filter masks (szg_mask / ScanMask): a masked search returns what the CPU oracle returns for the
same filter -- equal ids, bit-equal float64 distances -- and what the same search returns through allow=, on every
path a filter takes: one sweep per query (dense and selective form), shared sweeps, radius batches, the sketch
pre-pass, the exact replay, sharded handles, coalesced lone callers and the Collection mirror's cache.  The shapes
are the smallest at which each piece can still go wrong."""
import threading

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import (Collection, CollectionOptions, ScanIndex, SearchArgs, SzgError, SZG_COSINE, SZG_EUCLIDEAN, _lib,
                         pack_allow_bits)

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5
SEED = 0x53595A4700000000


def assert_same(rows, dist, o_rows, o_dist):
    assert len(rows) == len(o_rows)
    assert list(map(int, rows)) == list(map(int, o_rows)), "doc rows differ"
    d = np.asarray(dist, dtype=np.float64)
    od = np.asarray(o_dist, dtype=np.float64)
    both_nan = np.isnan(d) & np.isnan(od)
    ok = both_nan | (np.abs(d - od) <= REL_TOL * np.abs(od))
    assert ok.all(), (d, od)
    # stronger, expected: bit-identical float64
    assert (both_nan | (d == od)).all(), ("not bit-exact", d, od)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def random_allowed(n, rate, seed):
    return np.random.default_rng(seed).random(n) < rate


def check_topk(ix, rows, dim, bits, metric, Q, k, allowed, masks):
    """masks= against the oracle and against allow=.  allowed: one bool[n] per query (None = unfiltered)."""
    n = ix.rows
    Q = np.atleast_2d(Q)
    r, d, c = ix.search_topk(Q, k, masks=masks)
    A = np.stack([a if a is not None else np.ones(n, bool) for a in allowed])
    r2, d2, c2 = ix.search_topk(Q, k, allow=A)
    assert (c == c2).all() and (r == r2).all()
    assert (d.view(np.uint64) == d2.view(np.uint64)).all()
    for i in range(Q.shape[0]):
        o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, metric, Q[i], k=k, allow=A[i].astype(np.uint8))
        assert_same(r[i, : c[i]], d[i, : c[i]], o_rows, o_dist)


# ---- 1. mask objects ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 777, 1000])
def test_mask_objects(n, devices):
    dim, bits = 8, 8
    words = (n + 63) // 64
    with ScanIndex(dim, bits, SZG_COSINE, devices=devices) as ix:
        ix.load(orc.synth_rows(SEED, 0, n, dim, bits))
        a_bool, b_bool = random_allowed(n, 0.5, n), random_allowed(n, 0.3, n + 1)
        a, b = ix.mask(a_bool), ix.mask(b_bool)
        assert (a.read() == pack_allow_bits(a_bool)[0]).all() and a.count == int(a_bool.sum())
        assert a.count == popcount(a.read())
        # words with every bit set, the tail included: stored without the tail
        full = ix.mask(np.full((1, words), np.uint64(0xFFFFFFFFFFFFFFFF)))
        assert full.count == n and (full.read() == pack_allow_bits(np.ones(n, bool))[0]).all()
        empty = ix.mask(np.zeros(n, bool))
        assert empty.count == 0 and not empty.read().any()
        assert ix.mask_rows([]).count == 0
        # AND / OR / ANDNOT / NOT against numpy; NOT keeps the tail clear
        for got, want in (((a & b), a_bool & b_bool), ((a | b), a_bool | b_bool), (a.andnot(b), a_bool & ~b_bool),
                          ((~a), ~a_bool), ((~empty), np.ones(n, bool)), ((~full), np.zeros(n, bool))):
            assert (got.read() == pack_allow_bits(want)[0]).all()
            assert got.count == int(want.sum()) == popcount(got.read())
        assert (~a).count == n - a.count
        # row lists: duplicates, rows that share a word, the first and the last row
        listed = [0, n - 1, n - 1, 0] + [r for r in (1, 2, 2, 62, 63, 64, 64, 700) if r < n]
        m = ix.mask_rows(listed)
        want = np.zeros(n, bool)
        want[listed] = True
        assert (m.read() == pack_allow_bits(want)[0]).all() and m.count == int(want.sum())
        with pytest.raises(SzgError) as e:
            ix.mask_rows([0, n])
        assert e.value.code == _lib.SZG_E_RANGE
        st = ix.mask_stats()
        assert st["live_masks"] >= 5 and st["device_bytes"] > 0
        m.close()
        assert ix.mask_stats()["live_masks"] == st["live_masks"] - 1
    assert not a._h  # the index closed the masks it still held


# ---- 2. one sweep per query -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 32])
@pytest.mark.parametrize("metric", [SZG_EUCLIDEAN, SZG_COSINE])
@pytest.mark.parametrize("n", [777, 3000])
def test_one_sweep_per_query(bits, metric, n):
    dim = 17
    rows = orc.synth_rows(SEED + bits, 0, n, dim, bits)
    Q = orc.synth_vectors(SEED + 1, 0, 4, dim)
    with ScanIndex(dim, bits, metric) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        for rate in (0.5, 0.01):  # the dense form, the selective form
            allowed = [random_allowed(n, rate, 10 * j + int(rate * 100)) for j in range(4)]
            handles = [ix.mask(a) for a in allowed]
            for k in (1, 10):
                # ONE handle for the 4-query call: read in place
                ix.reset_stats()
                r, d, c = ix.search_topk(Q, k, masks=handles[0])
                st = ix.mask_stats()
                assert st["shared_batches"] >= 1 and st["h2d_bytes"] == 0 and st["d2d_bytes"] == 0
                check_topk(ix, rows, dim, bits, metric, Q, k, [allowed[0]] * 4, handles[0])
                # 4 entries that differ, one of them None: gathered card-to-card
                ix.reset_stats()
                mixed = [handles[0], None, handles[2], handles[3]]
                ix.search_topk(Q, k, masks=mixed)
                st = ix.mask_stats()
                assert st["d2d_bytes"] > 0 and st["h2d_bytes"] == 0
                check_topk(ix, rows, dim, bits, metric, Q, k, [allowed[0], None, allowed[2], allowed[3]], mixed)
        # the allow= path is the one that uploads
        ix.reset_stats()
        ix.search_topk(Q, 10, allow=np.stack(allowed))
        h2d, per_call = ix.mask_stats()["h2d_bytes"], 4 * ((n + 63) // 64) * 8
        assert h2d >= per_call and h2d % ((n + 63) // 64 * 8) == 0   # (more when a pre-pass hands queries over)


# ---- 3. shared sweeps -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("bits", [4, 8, 32, 64])
def test_shared_sweeps(bits, devices):
    dim, n, k, nq = 64, 3000, 10, 20
    rows = orc.synth_rows(SEED + 3 * bits, 0, n, dim, bits)
    Q = orc.synth_vectors(SEED + 2, 0, nq, dim)
    shards = len(devices) if devices else 1   # (every shard counts the queries its sweep served)
    with ScanIndex(dim, bits, SZG_COSINE, devices=devices) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 1)
        one_bool = random_allowed(n, 0.4, bits)
        one = ix.mask(one_bool)
        ix.reset_stats()
        check_topk(ix, rows, dim, bits, SZG_COSINE, Q, k, [one_bool] * nq, one)
        assert ix.mask_stats()["shared_batches"] >= 1
        ix.reset_stats()
        ix.search_topk(Q, k, masks=one)
        assert ix.stats()["mq_queries"] == nq * shards and ix.mask_stats()["h2d_bytes"] == 0
        per_bool = [random_allowed(n, 0.1 + 0.04 * j, 100 + j) if j % 5 else None for j in range(nq)]
        per = [ix.mask(a) if a is not None else None for a in per_bool]
        ix.reset_stats()
        ix.search_topk(Q, k, masks=per)
        assert ix.stats()["mq_queries"] == nq * shards
        st = ix.mask_stats()
        assert st["d2d_bytes"] > 0 and st["h2d_bytes"] == 0
        check_topk(ix, rows, dim, bits, SZG_COSINE, Q, k, per_bool, per)


# ---- 4. radius batches ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 32])
def test_radius_batch(bits):
    dim, n, nq = 32, 3000, 6
    rows = orc.synth_rows(SEED + 5 * bits, 0, n, dim, bits)
    Q = orc.synth_vectors(SEED + 3, 0, nq, dim)
    for metric in (SZG_EUCLIDEAN, SZG_COSINE):
        with ScanIndex(dim, bits, metric) as ix:
            ix.load(rows)
            shared_bool = random_allowed(n, 0.5, 7)
            mixed_bool = [random_allowed(n, 0.3 + 0.1 * j, 20 + j) if j != 2 else None for j in range(nq)]
            shared = ix.mask(shared_bool)
            mixed = [ix.mask(a) if a is not None else None for a in mixed_bool]
            for allowed, masks in (([shared_bool] * nq, shared), (mixed_bool, mixed)):
                A = np.stack([a if a is not None else np.ones(n, bool) for a in allowed])
                radii = [float(np.quantile(orc.all_distances(rows, dim, bits, metric, Q[i])[A[i]], 0.05)) for i in range(nq)]
                ix.reset_stats()
                got = ix.search_radius_batch(Q, radii, masks=masks)
                assert ix.mask_stats()["h2d_bytes"] == 0
                ref = ix.search_radius_batch(Q, radii, allow=A)
                for i in range(nq):
                    o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, metric, Q[i], radius=radii[i],
                                                         allow=A[i].astype(np.uint8))
                    assert len(o_rows) > 0
                    assert_same(got[i][0], got[i][1], o_rows, o_dist)
                    assert (got[i][0] == ref[i][0]).all() and (got[i][1] == ref[i][1]).all()
            # a lone radius search takes the handle too
            r1, d1 = ix.search_radius(Q[0], radii[0], masks=mixed[0])
            assert (r1 == got[0][0]).all() and (d1 == got[0][1]).all()


# ---- 5. sketch pre-pass -----------------------------------------------------------------------------------------------

def test_sketch_prepass():
    dim, n, k, bits = 32, 5000, 5, 32
    rows = orc.synth_rows(SEED + 9, 0, n, dim, bits)
    Q = orc.synth_vectors(SEED + 4, 0, 3, dim)
    allowed = random_allowed(n, 0.3, 5)
    with ScanIndex(dim, bits, SZG_COSINE) as ix:
        ix.load(rows)
        ix.set_option("sketch", 1)
        m = ix.mask(allowed)
        ix.reset_stats()
        for i in range(Q.shape[0]):
            check_topk(ix, rows, dim, bits, SZG_COSINE, Q[i], k, [allowed], m)
        assert ix.stats()["sketch_queries"] >= 1
        ix.reset_stats()
        ix.search_topk(Q[0], k, masks=m)
        st = ix.mask_stats()
        assert st["h2d_bytes"] == 0 and st["shared_batches"] >= 1


# ---- 6. ties and the exact replay -------------------------------------------------------------------------------------

def test_ties_take_the_full_replay():
    dim, bits = 6, 32
    base = orc.synth_vectors(SEED, 0, 4, dim)
    rows = orc.encode_rows(np.repeat(base, 300, axis=0), bits)  # 1200 rows, 4 distinct vectors
    q = base[2] + 0.01
    allowed = np.arange(1200) % 2 == 0
    for metric in (SZG_EUCLIDEAN, SZG_COSINE):
        with ScanIndex(dim, bits, metric) as ix:
            ix.load(rows)
            m = ix.mask(allowed)
            ix.reset_stats()
            r, d, c = ix.search_topk(q, 10, masks=m)
            assert ix.stats()["full_replays"] >= 1
            o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, metric, q, k=10, allow=allowed.astype(np.uint8))
            assert_same(r[0, : c[0]], d[0, : c[0]], o_rows, o_dist)
            check_topk(ix, rows, dim, bits, metric, q, 10, [allowed], m)


# ---- 7. mutations -----------------------------------------------------------------------------------------------------

def test_mutations():
    dim, bits, n, k, metric = 24, 32, 2000, 5, SZG_EUCLIDEAN
    rows = orc.synth_rows(SEED + 11, 0, n, dim, bits)
    q = orc.synth_vectors(SEED + 5, 0, 1, dim)[0]
    allowed = random_allowed(n, 0.5, 3)
    with ScanIndex(dim, bits, metric) as ix, ScanIndex(dim, bits, metric) as other:
        ix.load(rows)
        other.load(rows)
        m = ix.mask(allowed)
        r, d, c = ix.search_topk(q, k, masks=m)
        best = int(r[0, 0])
        assert allowed[best]
        # a tombstone is applied through the live bits: the mask stays valid, the hit is gone
        ix.tombstone(best)
        gone = allowed.copy()
        gone[best] = False
        r, d, c = ix.search_topk(q, k, masks=m)
        assert best not in r[0]
        o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, metric, q, k=k, allow=gone.astype(np.uint8))
        assert_same(r[0, : c[0]], d[0, : c[0]], o_rows, o_dist)
        # an overwritten allowed row is seen
        target = int(np.flatnonzero(gone)[-1])
        ix.overwrite_vector(target, q)
        r, d, c = ix.search_topk(q, k, masks=m)
        assert int(r[0, 0]) == target
        now = ix.read_rows(0, n)
        o_rows, o_dist, _ = orc.search_exact(now, dim, bits, metric, q, k=k, allow=gone.astype(np.uint8))
        assert_same(r[0, : c[0]], d[0, : c[0]], o_rows, o_dist)
        # a mask of another handle
        with pytest.raises(SzgError) as e:
            other.search_topk(q, k, masks=m)
        assert e.value.code == _lib.SZG_E_INVALID
        # appends and loads change the row count: older masks are stale, fresh ones work
        for mutate in (lambda: ix.append(rows[:70]), lambda: ix.load(rows[:1500])):
            mutate()
            for call in (lambda: ix.search_topk(q, k, masks=m), lambda: ix.search_radius_batch(q, 1.0, masks=m),
                         lambda: m & m, lambda: ~m):
                with pytest.raises(SzgError) as e:
                    call()
                assert e.value.code == _lib.SZG_E_INVALID and "stale" in str(e.value)
            assert m.count == int(allowed.sum()) and (m.read() == pack_allow_bits(allowed)[0]).all()  # still readable
            fresh_bool = random_allowed(ix.rows, 0.5, ix.rows)
            if best < ix.rows:
                fresh_bool[best] = False   # (tombstoned before the append; the load brought every row back)
            fresh = ix.mask(fresh_bool)
            r, d, c = ix.search_topk(q, k, masks=fresh)
            o_rows, o_dist, _ = orc.search_exact(ix.read_rows(0, ix.rows), dim, bits, metric, q, k=k,
                                                 allow=fresh_bool.astype(np.uint8))
            assert_same(r[0, : c[0]], d[0, : c[0]], o_rows, o_dist)
            m.close()
            m, allowed = fresh, fresh_bool


# ---- 8. concurrent lone callers ---------------------------------------------------------------------------------------

def test_concurrent_lone_callers_share_the_handle():
    dim, bits, n, k, nt = 64, 32, 20000, 10, 8
    rows = orc.synth_rows(SEED + 13, 0, n, dim, bits)
    Q = orc.synth_vectors(SEED + 6, 0, nt, dim)
    allowed = random_allowed(n, 0.25, 9)
    with ScanIndex(dim, bits, SZG_COSINE) as ix:
        ix.load(rows)
        m = ix.mask(allowed)
        serial = [ix.search_topk(Q[i], k, allow=allowed) for i in range(nt)]
        ix.reset_stats()
        start = threading.Barrier(nt)
        out, errs = [None] * nt, []

        def caller(t):
            try:
                start.wait()
                out[t] = ix.search_topk(Q[t], k, masks=m)
            except BaseException as e:  # noqa: B902
                errs.append(e)
                start.abort()
        th = [threading.Thread(target=caller, args=(t,)) for t in range(nt)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs
        assert ix.mask_stats()["h2d_bytes"] == 0 and ix.stats()["queries"] == nt
        for t in range(nt):
            assert (out[t][0] == serial[t][0]).all() and (out[t][1] == serial[t][1]).all()
            o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, SZG_COSINE, Q[t], k=k, allow=allowed.astype(np.uint8))
            assert_same(out[t][0][0], out[t][1][0], o_rows, o_dist)


# ---- 9. the Collection mirror -----------------------------------------------------------------------------------------

def test_collection_mirror_passes_handles():
    dim, n, k = 16, 600, 5
    V = orc.synth_vectors(SEED + 15, 0, n, dim)
    Q = orc.synth_vectors(SEED + 7, 0, 8, dim)
    c = Collection(CollectionOptions(Name="masks", DistanceMethod=1, DimensionCount=dim, Quantization=32))
    c.AddDocuments(range(n), V, [b"m%d" % i for i in range(n)])

    def third(i, meta):
        return i % 3 == 0
    ids = lambda res: [(r.ID, r.Distance) for r in res.Results]  # noqa: E731
    first = c.Search(SearchArgs(Vector=Q[0], K=k, Filter=third, FilterKey="third", Precision="exact"))
    c._index.reset_stats()
    second = c.Search(SearchArgs(Vector=Q[0], K=k, Filter=lambda i, m: 1 / 0, FilterKey="third", Precision="exact"))
    assert c._index.mask_stats()["h2d_bytes"] == 0
    unkeyed = c.Search(SearchArgs(Vector=Q[0], K=k, Filter=third, Precision="exact"))
    assert ids(first) == ids(second) == ids(unkeyed) and all(r.ID % 3 == 0 for r in first.Results)
    c._index.reset_stats()
    batch = c.SearchBatch([SearchArgs(Vector=Q[i], K=k, Filter=third, FilterKey="third", Precision="exact") for i in range(8)])
    st = c._index.mask_stats()
    assert st["shared_batches"] >= 1 and st["h2d_bytes"] == 0
    plain = c.SearchBatch([SearchArgs(Vector=Q[i], K=k, Filter=third, Precision="exact") for i in range(8)])
    assert [ids(b) for b in batch] == [ids(p) for p in plain]
    rad = c.Search(SearchArgs(Vector=Q[1], Radius=0.45, Filter=third, FilterKey="third", Precision="exact"))
    rad2 = c.Search(SearchArgs(Vector=Q[1], Radius=0.45, Filter=third, Precision="exact"))
    assert ids(rad) == ids(rad2) and all(r.ID % 3 == 0 for r in rad.Results)
    # the version moves: the old entry's device mask is closed, the new verdicts apply
    live = c._index.mask_stats()["live_masks"]
    c.removeDocument(first.Results[0].ID)
    after = c.Search(SearchArgs(Vector=Q[0], K=k, Filter=third, FilterKey="third", Precision="exact"))
    assert first.Results[0].ID not in [r.ID for r in after.Results]
    assert c._index.mask_stats()["live_masks"] <= live
    c.Close()
