"""Compaction and reorder of the resident rows on the device (szg_index_compact / szg_index_reorder,
ScanIndex.compact / reorder, Collection.Compact): the rows that remain are byte for byte the ones that were kept, a
compacted index answers as the CPU oracle does on those rows -- equal ids, bit-equal float64 distances -- and as a
fresh index loaded with them, masks carried across the call hold the bits of the rows that moved, and an index without
tombstones is back on the unmasked fast path.  The shapes are the smallest that cross each boundary the gather
addresses by: 16-row tiles, 64-row mask words, linear against tiled layout, rows that are no multiple of 16 bytes."""
import functools

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import (Collection, CollectionOptions, ScanIndex, SearchArgs, SzgError, SZG_COSINE, SZG_EUCLIDEAN, _lib,
                         pack_allow_bits)

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5
SEED = 0x53595A4700000000
DROPPED = np.uint64(0xFFFFFFFFFFFFFFFF)
# bits, dim: 4 x 128 and 8 x 64 are tiled; 8 x 17 is linear with a padded pitch; the others linear
LAYOUTS = [(4, 128), (8, 64), (8, 17), (16, 17), (32, 17), (64, 5)]


@functools.lru_cache(maxsize=None)
def corpus(bits, dim, n):
    rows = orc.synth_rows(SEED + bits, 0, n, dim, bits)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def queries(dim, nq=4):
    return orc.synth_vectors(SEED + 1, 0, nq, dim)


def assert_same(rows, dist, o_rows, o_dist):
    assert len(rows) == len(o_rows)
    assert list(map(int, rows)) == list(map(int, o_rows)), "doc rows differ"
    d = np.asarray(dist, dtype=np.float64)
    od = np.asarray(o_dist, dtype=np.float64)
    both_nan = np.isnan(d) & np.isnan(od)
    assert (both_nan | (np.abs(d - od) <= REL_TOL * np.abs(od))).all(), (d, od)
    assert (both_nan | (d == od)).all(), ("not bit-exact", d, od)   # stronger, expected: bit-identical float64


def dead_rows(n, seed, whole=True):
    """A seeded random third of the rows, row 0 and the last row; with `whole` (n >= 64) also one whole 16-row tile
    and one whole 64-row word."""
    rng = np.random.default_rng(seed)
    dead = np.zeros(n, bool)
    dead[rng.choice(n, n // 3, replace=False)] = True
    dead[0] = dead[n - 1] = True
    if whole and n >= 64:
        dead[16:32] = True
        w = (n // 64 - 1) * 64
        dead[w:w + 64] = True
    return dead


def tombstone(ix, dead):
    for r in np.flatnonzero(dead):
        ix.tombstone(int(r))


def check_bytes(ix, rows, dead):
    """compact() after the tombstones of `dead`: the rows, the counts and the map."""
    live = ~dead
    tombstone(ix, dead)
    new_of_old = ix.compact()
    want = np.full(len(rows), DROPPED, dtype=np.uint64)
    want[live] = np.arange(int(live.sum()), dtype=np.uint64)
    assert ix.rows == ix.live_rows == int(live.sum())
    assert (ix.read_rows(0, ix.rows) == rows[live]).all()
    assert new_of_old.dtype == np.uint64 and (new_of_old == want).all()


def check_topk(ix, rows_now, dim, bits, metric, Q, k, fresh=None, allowed=None, masks=None):
    """The index against the oracle on rows_now (allowed: bool[rows], the filter and / or the live rows) and, word
    for word, against `fresh`, an index loaded with the same rows."""
    r, d, c = ix.search_topk(Q, k, masks=masks)
    allow = allowed.astype(np.uint8) if allowed is not None else None
    for i in range(Q.shape[0]):
        o_rows, o_dist, _ = orc.search_exact(rows_now, dim, bits, metric, Q[i], k=k, allow=allow)
        assert_same(r[i, : c[i]], d[i, : c[i]], o_rows, o_dist)
    if fresh is not None:
        r2, d2, c2 = fresh.search_topk(Q, k, allow=None if allowed is None else np.tile(allowed, (Q.shape[0], 1)))
        assert (c == c2).all() and (r == r2).all() and (d.view(np.uint64) == d2.view(np.uint64)).all()
    return r, d, c


def check_radius(ix, rows_now, dim, bits, metric, Q, fresh):
    radii = [float(np.quantile(orc.all_distances(rows_now, dim, bits, metric, Q[i]), 0.05)) for i in range(Q.shape[0])]
    got = ix.search_radius_batch(Q, radii)
    ref = fresh.search_radius_batch(Q, radii)
    for i in range(Q.shape[0]):
        o_rows, o_dist, _ = orc.search_exact(rows_now, dim, bits, metric, Q[i], radius=radii[i])
        assert len(o_rows) > 0
        assert_same(got[i][0], got[i][1], o_rows, o_dist)
        assert (got[i][0] == ref[i][0]).all() and (got[i][1].view(np.uint64) == ref[i][1].view(np.uint64)).all()


def check_answers(bits, metric, multi_query, n, devices=None):
    dim, k = 17, 10
    rows, Q = corpus(bits, dim, n), queries(dim)
    dead = dead_rows(n, n + bits)
    kept = rows[~dead]
    with ScanIndex(dim, bits, metric, devices=devices) as ix, ScanIndex(dim, bits, metric, devices=devices) as fresh:
        for h in (ix, fresh):
            if multi_query is not None:
                h.set_option("multi_query", multi_query)
        ix.load(rows)
        tombstone(ix, dead)
        ix.compact()
        fresh.load(kept)
        check_topk(ix, kept, dim, bits, metric, Q, k, fresh=fresh)
        check_radius(ix, kept, dim, bits, metric, Q, fresh)


def check_masks(n, op, devices=None, bits=8):
    """Two masks carried and one not, across compact() or a reorder()."""
    dim, k, metric = 17, 5, SZG_COSINE
    rows, Q = corpus(bits, dim, n), queries(dim)
    dead = dead_rows(n, 3 * n, whole=False)
    rng = np.random.default_rng(n)
    if op == "compact":
        src = np.flatnonzero(~dead)
    else:
        src = rng.permutation(np.flatnonzero(~dead))[: max(1, int((~dead).sum()) * 2 // 3)]
    a_bool, b_bool, c_bool = (rng.random(n) < p for p in (0.5, 0.1, 0.5))
    with ScanIndex(dim, bits, metric, devices=devices) as ix:
        ix.load(rows)
        tombstone(ix, dead)
        a, b, c = ix.mask(a_bool), ix.mask(b_bool), ix.mask(c_bool)
        # a stale mask in carry is refused, and nothing moved
        with ScanIndex(dim, bits, metric, devices=devices) as other:
            other.load(rows)
            stale = other.mask(a_bool)
            other.append(rows[:1])
            with pytest.raises(SzgError) as e:
                other.compact(carry=[stale]) if op == "compact" else other.reorder(src, carry=[stale])
            assert e.value.code == _lib.SZG_E_INVALID and "stale mask" in str(e.value)
            assert other.rows == n + 1 and (other.read_rows(0, n) == rows).all()
            with pytest.raises(SzgError) as e:   # a mask of another handle
                ix.compact(carry=[stale]) if op == "compact" else ix.reorder(src, carry=[stale])
            assert e.value.code == _lib.SZG_E_INVALID
            assert ix.rows == n and ix.live_rows == int((~dead).sum())
        live_masks = ix.mask_stats()["live_masks"]
        if op == "compact":
            ix.compact(carry=[a, b])
        else:
            ix.reorder(src, carry=[a, b])
        m = len(src)
        assert ix.rows == ix.live_rows == m and (ix.read_rows(0, m) == rows[src]).all()
        assert ix.mask_stats()["live_masks"] == live_masks
        for mask, old in ((a, a_bool), (b, b_bool)):
            words = mask.read()
            assert (words == pack_allow_bits(old[src])[0]).all()   # (tail bits clear: pack_allow_bits pads with 0)
            assert mask.count == int(old[src].sum())
            ix.reset_stats()
            check_topk(ix, rows[src], dim, bits, metric, Q, k, allowed=old[src], masks=mask)
            assert ix.mask_stats()["h2d_bytes"] == 0
        both = a & b   # carried masks combine with each other and with masks made afterwards
        assert (both.read() == pack_allow_bits((a_bool & b_bool)[src])[0]).all()
        assert ((a | ix.mask(np.ones(m, bool))).count) == m
        for call in (lambda: ix.search_topk(Q, k, masks=c), lambda: c & a, lambda: ~c):
            with pytest.raises(SzgError) as e:
                call()
            assert e.value.code == _lib.SZG_E_INVALID and "stale mask" in str(e.value)
        assert c.count == int(c_bool.sum()) and (c.read() == pack_allow_bits(c_bool)[0]).all()   # still readable


# ---- 1. bytes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 777, 3000])
@pytest.mark.parametrize("bits,dim", LAYOUTS)
def test_compact_bytes(bits, dim, n):
    rows = corpus(bits, dim, n)
    for whole in ((True, False) if n >= 64 else (True,)):   # (n = 64, 65: the whole word leaves no row; also without)
        with ScanIndex(dim, bits, SZG_COSINE) as ix:
            ix.load(rows)
            check_bytes(ix, rows, dead_rows(n, 7 * n + bits, whole))


@pytest.mark.parametrize("bits,dim", [(8, 64), (32, 17)])
def test_compact_everything_tombstoned_then_append(bits, dim):
    n, k = 100, 5
    rows, Q = corpus(bits, dim, n), queries(dim)
    with ScanIndex(dim, bits, SZG_EUCLIDEAN) as ix:
        ix.load(rows)
        tombstone(ix, np.ones(n, bool))
        new_of_old = ix.compact()
        assert ix.rows == ix.live_rows == 0 and (new_of_old == DROPPED).all()
        r, d, c = ix.search_topk(Q, k)
        assert not c.any()
        ix.append(rows[:70])
        assert ix.rows == ix.live_rows == 70 and (ix.read_rows(0, 70) == rows[:70]).all()
        check_topk(ix, rows[:70], dim, bits, SZG_EUCLIDEAN, Q, k)


def test_compact_without_tombstones_is_a_no_op():
    bits, dim, n, k = 8, 64, 300, 5
    rows, Q = corpus(bits, dim, n), queries(dim)
    allowed = np.random.default_rng(5).random(n) < 0.5
    with ScanIndex(dim, bits, SZG_COSINE) as ix:
        ix.load(rows)
        m = ix.mask(allowed)
        new_of_old = ix.compact()
        assert (new_of_old == np.arange(n, dtype=np.uint64)).all() and ix.rows == ix.live_rows == n
        check_topk(ix, rows, dim, bits, SZG_COSINE, Q, k, allowed=allowed, masks=m)   # the mask is not stale


# ---- 2. answers -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("multi_query", [0, None])
@pytest.mark.parametrize("metric", [SZG_EUCLIDEAN, SZG_COSINE])
@pytest.mark.parametrize("bits", [8, 32])
def test_compacted_answers(bits, metric, multi_query):
    check_answers(bits, metric, multi_query, 3000)


# ---- 3. the fast path is back ---------------------------------------------------------------------------------------

def test_fast_path_restored():
    """One tombstone makes every launch of the shard a masked one: the grouped 8-bit sweep (4 queries per row read)
    falls back to one query per row read.  compact() brings it back.  (scan_group_plan -- szg_debug_scan_group --
    gives 1 pass for the unmasked and 4 for the masked launch of these 4 queries.)"""
    bits, dim, n, k = 8, 64, 3000, 10
    rows, Q = corpus(bits, dim, n), queries(dim)
    row_bytes = dim

    def swept(ix):
        ix.reset_stats()
        ix.search_topk(Q, k)
        st = ix.stats()
        print("scan_bytes", st["scan_bytes"], "escalations", st["escalations"], "rows", ix.rows)
        return st["scan_bytes"]
    with ScanIndex(dim, bits, SZG_COSINE) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        assert swept(ix) == 1 * n * row_bytes
        ix.tombstone(1234)
        assert swept(ix) == 4 * n * row_bytes
        ix.compact()
        assert ix.rows == n - 1
        assert swept(ix) == 1 * (n - 1) * row_bytes
        check_topk(ix, np.delete(rows, 1234, axis=0), dim, bits, SZG_COSINE, Q, k)


# ---- 4. reorder -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,dim", [(8, 64), (32, 17)])
def test_reorder(bits, dim):
    n, k, metric = 777, 10, SZG_COSINE
    rows, Q = corpus(bits, dim, n), queries(dim)
    dead = dead_rows(n, 11 + bits, whole=False)
    live = np.flatnonzero(~dead)
    rng = np.random.default_rng(bits)
    src = rng.permutation(live)[: len(live) * 2 // 3]
    with ScanIndex(dim, bits, metric) as ix, ScanIndex(dim, bits, metric) as fresh:
        ix.load(rows)
        tombstone(ix, dead)
        before = ix.search_topk(Q, k)
        for bad, code in ((np.append(src, src[3]), _lib.SZG_E_INVALID), (np.append(src, n), _lib.SZG_E_RANGE),
                          (np.append(src, np.flatnonzero(dead)[5]), _lib.SZG_E_INVALID),
                          (np.array([n + 5]), _lib.SZG_E_RANGE)):
            with pytest.raises(SzgError) as e:
                ix.reorder(bad)
            assert e.value.code == code
            assert ix.rows == n and ix.live_rows == len(live) and (ix.read_rows(0, n) == rows).all()
            after = ix.search_topk(Q, k)
            assert all((x == y).all() for x, y in zip(before, after))
        ix.reorder(src)
        assert ix.rows == ix.live_rows == len(src)
        assert (ix.read_rows(0, len(src)) == rows[src]).all()
        fresh.load(rows[src])
        check_topk(ix, rows[src], dim, bits, metric, Q, k, fresh=fresh)
        check_radius(ix, rows[src], dim, bits, metric, Q, fresh)
        ix.reorder([])   # n_rows == 0 empties the index
        assert ix.rows == ix.live_rows == 0


# ---- 5. masks -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ["compact", "reorder"])
@pytest.mark.parametrize("n", [65, 777])
def test_carried_masks(n, op):
    check_masks(n, op)


# ---- 6. several shards ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,dim", [(8, 64), (32, 17)])
def test_sharded_bytes(bits, dim):
    n = 1000
    rows = corpus(bits, dim, n)
    with ScanIndex(dim, bits, SZG_COSINE, devices=[0, 0]) as ix:
        ix.load(rows)
        check_bytes(ix, rows, dead_rows(n, 13 + bits))
        # rows of both shards interleaved: the runs of a reorder
        now = rows[~dead_rows(n, 13 + bits)]
        src = np.random.default_rng(bits).permutation(len(now))[:400]
        ix.reorder(src)
        assert ix.rows == ix.live_rows == 400 and (ix.read_rows(0, 400) == now[src]).all()


def test_sharded_reorder_in_several_windows():
    """Rows cross the devices through a 64 MiB stage: 24 000 rows of 6 144 bytes make each destination shard more than
    one window, and a random permutation interleaves the two source shards row by row."""
    bits, dim, n = 64, 768, 24000
    with ScanIndex(dim, bits, SZG_COSINE, devices=[0, 0]) as ix:
        ix.synth(n, SEED + 21)
        rows = ix.read_rows(0, n)
        src = np.random.default_rng(21).permutation(n)[: n - 500]
        ix.reorder(src)
        assert ix.rows == ix.live_rows == len(src)
        assert (ix.read_rows(0, len(src)) == rows[src]).all()


@pytest.mark.parametrize("bits", [8, 32])
def test_sharded_answers(bits):
    check_answers(bits, SZG_COSINE, None, 1000, devices=[0, 0])


@pytest.mark.parametrize("op", ["compact", "reorder"])
@pytest.mark.parametrize("bits", [8, 32])
def test_sharded_masks(bits, op):
    check_masks(1000, op, devices=[0, 0], bits=bits)


# ---- 7. sketch ------------------------------------------------------------------------------------------------------

def test_sketch_is_rebuilt():
    dim, n, k, bits = 32, 5000, 5, 32
    rows = corpus(bits, dim, n)
    Q = queries(dim, 3)
    dead = np.zeros(n, bool)
    dead[np.random.default_rng(9).choice(n, 500, replace=False)] = True
    with ScanIndex(dim, bits, SZG_COSINE) as ix:
        ix.load(rows)
        ix.set_option("sketch", 1)
        ix.set_option("sketch_min_rows", 1024)
        for i in range(Q.shape[0]):
            check_topk(ix, rows, dim, bits, SZG_COSINE, Q[i: i + 1], k)
        first = ix.stats()["sketch_queries"]
        assert first >= 1
        tombstone(ix, dead)
        ix.compact()
        for i in range(Q.shape[0]):
            check_topk(ix, rows[~dead], dim, bits, SZG_COSINE, Q[i: i + 1], k)
        assert ix.stats()["sketch_queries"] > first


# ---- 8. appends after a compaction ----------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,dim", [(8, 64), (32, 17)])
def test_appends_after_compaction(bits, dim):
    n, k = 777, 10
    rows, Q = corpus(bits, dim, n), queries(dim)
    dead = dead_rows(n, 17 + bits)
    with ScanIndex(dim, bits, SZG_EUCLIDEAN) as ix:
        ix.load(rows)
        tombstone(ix, dead)
        ix.compact()
        extra = orc.synth_rows(SEED + 99, 0, 70, dim, bits)
        ix.append(extra)
        now = np.concatenate([rows[~dead], extra])
        assert ix.rows == len(now) and (ix.read_rows(0, ix.rows) == now).all()
        gone = len(now) - 30
        ix.tombstone(gone)
        allowed = np.ones(len(now), bool)
        allowed[gone] = False
        assert ix.live_rows == len(now) - 1
        check_topk(ix, now, dim, bits, SZG_EUCLIDEAN, Q, k, allowed=allowed)


# ---- 9. the Collection mirror ---------------------------------------------------------------------------------------

def ids_of(res):
    return [(r.ID, r.Distance, r.Metadata) for r in res.Results]


def test_collection_compact_carries_the_cached_filters():
    dim, n, k = 16, 600, 5
    V = orc.synth_vectors(SEED + 15, 0, n, dim)
    Q = queries(dim, 2)
    c = Collection(CollectionOptions(Name="compact", DistanceMethod=1, DimensionCount=dim, Quantization=32))
    c.AddDocuments(range(n), V, [b"m%d" % i for i in range(n)])
    calls = [0]

    def third(i, meta):
        calls[0] += 1
        return i % 3 == 0
    removed = list(range(0, 400, 2))
    for i in removed:
        c.removeDocument(i)

    def searches():
        return [ids_of(c.Search(SearchArgs(Vector=Q[0], K=k, Precision="exact"))),
                ids_of(c.Search(SearchArgs(Vector=Q[0], K=k, Filter=third, FilterKey="third", Precision="exact"))),
                ids_of(c.Search(SearchArgs(Vector=Q[1], K=k, Filter=third, Precision="exact"))),
                ids_of(c.Search(SearchArgs(Vector=Q[1], Radius=0.45, Filter=third, FilterKey="third", Precision="exact")))]
    before = searches()
    assert all(before) and all(i % 3 == 0 and i not in removed for i, _, _ in before[1])
    n_calls = calls[0]
    c._index.reset_stats()
    assert c.Compact() == len(removed)
    assert c._index.rows == c._index.live_rows == n - len(removed) == c.GetDocumentCount()
    assert searches() == before
    assert calls[0] == n_calls                          # the filter was not evaluated again
    assert c._index.mask_stats()["h2d_bytes"] == 0      # ... and nothing was uploaded
    assert c.Compact() == 0
    doc = c.GetDocument(401)
    assert doc.Metadata == b"m401" and (doc.Vector == V[401].astype(np.float32)).all()
    c.AddDocument(0, V[0], b"back")
    assert c.Search(SearchArgs(Vector=V[0], K=1, Precision="exact")).Results[0].ID == 0
    c.Close()


def test_collection_auto_compact():
    dim, n = 8, 100
    V = orc.synth_vectors(SEED + 16, 0, n, dim)
    c = Collection(CollectionOptions(Name="auto", DistanceMethod=0, DimensionCount=dim, Quantization=8), auto_compact=0.25)
    c.AddDocuments(range(n), V)
    for i in range(25):
        c.removeDocument(i)
    assert c.compactions == 0 and c._index.rows == n and c._index.live_rows == n - 25   # 25 of 100: not beyond a quarter
    c.removeDocument(25)
    assert c.compactions == 1 and c._index.rows == c._index.live_rows == n - 26
    res = c.Search(SearchArgs(Vector=V[60], K=1, Precision="exact"))
    assert res.Results[0].ID == 60
    c.Close()
    never = Collection(CollectionOptions(Name="never", DistanceMethod=0, DimensionCount=dim, Quantization=8))
    never.AddDocuments(range(n), V)
    for i in range(90):
        never.removeDocument(i)
    assert never.compactions == 0 and never._index.rows == n
    never.Close()


def test_strict_order_repages_once_through_reorder():
    """Ids appended out of string order and an answer with a tie: the mirror re-pages once -- on the card now -- and
    returns the reference's tie order."""
    dim, bits = 4, 8
    base = np.random.default_rng(11).uniform(-1, 1, (3, dim))
    ids = [5, 40, 100, 2, 31, 7, 1000, 12, 3, 64, 9, 77, 8, 200, 30, 6]
    vec = {id: base[i % 3] for i, id in enumerate(ids)}
    q = base[1] + 0.01
    c = Collection(CollectionOptions(Name="ties", DistanceMethod=1, DimensionCount=dim, Quantization=bits))
    for id in ids:
        c.AddDocument(id, vec[id], b"m%d" % id)
    c.removeDocument(31)
    left = [i for i in ids if i != 31]
    order = sorted(left, key=str)
    rows = orc.encode_rows(np.stack([vec[i] for i in order]), bits)
    for k in (2, 4, 5):
        want_rows, want_d, _ = orc.search_exact(rows, dim, bits, 1, q, k=k)
        got = c.Search(SearchArgs(Vector=q, K=k, Precision="exact"))
        assert [r.ID for r in got.Results] == [order[int(r)] for r in want_rows]
        assert [r.Distance for r in got.Results] == list(want_d)
    assert c.resorts == 1
    assert c._index.rows == c._index.live_rows == len(left)   # the re-page dropped the tombstoned row
    assert (c._index.read_rows(0, len(left)) == rows).all()
    c.Close()
