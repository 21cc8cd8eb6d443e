"""The matrix sketch sweep's masked forms (option sketch_masked; kernels_scan_mx.hip with -DSZG_MX_MASKED): top-k launches
of the sketch pre-pass with tombstones, one resident mask for every query, per-query resident masks or raw allow words
take the matrix sweep -- one block, wide, shared -- and skip the tiles none of whose rows is eligible.

Per leg, on handles opened with sketch_masked = 1: the answers and float64 distances == the oracle with allow=, the
certificate chain with eligible= (cert_check), the same answers under sketch_masked = 0 and sketch = 0, at least one
masked matrix launch on the counters (szg_debug_sketch_masked) -- every one of them with the tile skip where the
launch's eligibility is wave-uniform -- none under sketch_masked = 0, and the pass count of szg_stats.scan_bytes under
the rule of test_gpu_sketch_matrix.assert_pass_count: the matrix plan's 1 / 2 / 2 / 4 passes at 3 / 16 / 17 / 40 queries
with the option, one pass per query without (exact where the sketch settled every query, modulo 4 and not below
otherwise; at 40 queries both counts are 0 modulo 4, so only the settled form tells them apart).
"""
import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import Collection, CollectionOptions, Field, SearchArgs, _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import scan_masked_plan

import test_gpu_sketch_matrix as tsm
import test_gpu_sketch_share as tss
import test_gpu_sketch_wide as tsw

pytestmark = pytest.mark.gpu

SEED = 0x53595A4700011000
EUC, COS = tsm.EUC, tsm.COS
MID = tsm.MID
POOL = tsm.POOL
WAVES = 4   # waves per block of the sketch sweeps


def open_masked(dim, metric, devices=None, **options):
    return tsm.open_sketched(dim, metric, devices=devices, **dict({"sketch_masked": 1}, **options))


def eligible_2d(eligible, nq, n):
    return np.broadcast_to(np.ones(n, dtype=bool) if eligible is None else np.asarray(eligible, dtype=bool), (nq, n))


def assert_answers_per_query(got, corpus, Q, k, eligible, what):
    """tsm.assert_answers with one eligibility row per query."""
    r, d, cnt = got
    el = eligible_2d(eligible, len(Q), corpus.n)
    want = POOL.map(lambda a: orc.search_exact(corpus.packed, corpus.dim, 32, corpus.metric, a[0], k=k,
                                               allow=a[1].astype(np.uint8))[:2], zip(Q, el))
    for qi, (w_rows, w_dist) in enumerate(want):
        assert cnt[qi] == len(w_rows), ("count differs", what, qi, cnt[qi], len(w_rows))
        assert [int(x) for x in r[qi, : cnt[qi]]] == [int(x) for x in w_rows], ("rows differ", what, qi)
        g = d[qi, : cnt[qi]]
        assert ((g == w_dist) | (np.isnan(g) & np.isnan(w_dist))).all(), ("distances not bit-equal", what, qi)
        assert (r[qi, cnt[qi]:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), ("padding", what, qi)


def certified(ix, corpus, Q, k, what, eligible, dists=None, **filt):
    """tsm.certified_call where one eligibility serves every query; with per-query eligibility the same chain with the
    oracle asked query by query.  -> (answers, stats, dists)"""
    el = None if eligible is None else np.asarray(eligible, dtype=bool)
    if el is None or el.ndim == 1:
        got, st, _, _, dists = tsm.certified_call(ix, corpus, Q, k, what, dists=dists, eligible=el, **filt)
        return got, st, dists
    ix.reset_stats()
    got = ix.search_topk(Q, k, **filt)
    st = ix.stats()
    recs, ents, dropped = ix.certificates()
    sk = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]
    assert sorted(int(x) for x in sk["query"]) == list(range(Q.shape[0])), ("one sketch record per query", what)
    info = ix.sketch_info()
    assert info["in_sync"] == 1, (what, info)
    sk_corpus = cc.Corpus(ix.sketch_rows()[0], corpus.dim, 8, corpus.metric)
    if dists is None:
        dists = np.stack(list(POOL.map(lambda q: orc.all_distances(corpus.packed, corpus.dim, 32, corpus.metric, q), Q)))
    s = cc.check(corpus, Q, recs, ents, dropped, eligible=el, dists=dists, margins=tsm.MARGINS, what=what,
                 sketch=(sk_corpus, info["gscale"], info["exc_rows"]))
    assert s.skipped == 0, (what, sorted(s.skipped_rows)[:8])
    assert_answers_per_query(got, corpus, Q, k, el, what)
    return got, st, dists


def leg(ix, corpus, Q, k, what, eligible, want_on, skip, **filt):
    """One masked call three ways (see the module's docstring).  want_on: the sketch passes under sketch_masked = 1;
    skip: every masked launch of the call has wave-uniform eligibility."""
    n, dim, nq = corpus.n, corpus.dim, Q.shape[0]
    ix.set_option("sketch_masked", 1)
    got, st, dists = certified(ix, corpus, Q, k, what + ("on",), eligible, **filt)
    info = ix.sketch_masked_info()
    print(what, "masked launches", info, "stats", {x: st[x] for x in ("scan_launches", "scan_bytes", "sketch_queries", "escalations", "full_replays")})
    assert info["launches"] >= 1 and info["queries"] >= 3, ("no masked matrix launch", what, info)
    assert info["skip_launches"] == (info["launches"] if skip else 0), ("tile skip", what, info)
    tsm.assert_pass_count(st, n, dim, nq, want_on, what + ("on",))
    ix.set_option("sketch_masked", 0)
    got0, st0, _ = certified(ix, corpus, Q, k, what + ("off",), eligible, dists=dists, **filt)
    info0 = ix.sketch_masked_info()
    assert info0 == {"launches": 0, "skip_launches": 0, "queries": 0}, (what, info0)
    assert tsm.same(got, got0), ("answers differ from sketch_masked = 0", what)
    tsm.assert_pass_count(st0, n, dim, nq, nq, what + ("off",))   # today's count: one pass per query
    ix.set_option("sketch", 0)
    got00 = ix.search_topk(Q, k, **filt)
    assert tsm.same(got, got00), ("answers differ from sketch = 0", what)
    ix.certificates()   # (that call's records: read and dropped, the next leg checks its own)
    ix.set_option("sketch", 1)
    ix.set_option("sketch_masked", 1)
    return got


def test_plans_of_this_file():
    assert [tsm.matrix_passes(q) for q in (3, 16, 17, 40)] == [1, 2, 2, 4]
    # modulo 4 the matrix plan differs from one pass per query at 3, 16 and 17 queries, not at 40
    assert [(tsm.matrix_passes(q) - q) % 4 != 0 for q in (3, 16, 17, 40)] == [True, True, True, False]
    for dim in (64, 384, 768):
        for n_l in (3, 4, 12, 13, 16):
            assert scan_masked_plan(dim, 8, n_l, sketch_masked=1)["serves"]
            assert not scan_masked_plan(dim, 8, n_l, sketch_masked=0)["serves"]


# (dim, rows, queries, k, metric): every value of every axis, spread as test_gpu_sketch_matrix.CASES spreads them
CASES = [
    (64, 15, 3, 10, COS), (64, 16, 17, 1, EUC), (64, 17, 40, 10, EUC), (64, "s1", 16, 10, COS), (64, "s3", 3, 1, EUC),
    (384, 16, 40, 10, COS), (384, 15, 16, 10, EUC), (384, 17, 3, 10, COS), (384, "s1", 17, 1, COS), (384, "s3", 40, 10, EUC),
    (768, 15, 17, 10, EUC), (768, 17, 3, 1, COS), (768, 16, 40, 10, COS), (768, "s1", 16, 10, COS), (768, "s3", 17, 10, EUC),
]


def case_id(c):
    return tsm.case_id(c)


def masks_of(n, nq, rng):
    """Per-query eligibility that differs from query to query, densities from 0.9 down to 0.05, one None entry."""
    out = []
    for j in range(nq):
        if j == 1:
            out.append(None)
            continue
        m = rng.random(n) < (0.9, 0.5, 0.05)[j % 3]
        m[rng.integers(n)] = True
        out.append(m)
    return out


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_mask_legs(case):
    """Legs 1 - 5: tombstones (row 0, row n - 1, a whole tile), one resident mask for every query, per-query resident
    masks with a None entry, per-query raw allow words, tombstones combined with per-query masks."""
    dim, rows, nq, k, metric = case
    n = tsm.n_rows_of(dim, rows)
    seed = SEED + dim * 100 + (n % 1000) + k
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    rng = np.random.default_rng(seed & 0xFFFF)
    what = ("masked", case_id(case), "rows", n)
    want = tsm.matrix_passes(nq)
    lst = 8 if isinstance(rows, int) and k == 1 else 0
    with open_masked(dim, metric, sketch_list=lst) as ix:
        ix.synth(n, seed)
        # (2) one resident mask, passed with n_masks == 1
        shared = rng.random(n) < 0.6
        shared[[0, n - 1]] = True
        with ix.mask(shared) as m:
            leg(ix, corpus, Q, k, what + ("one mask",), shared, want, True, masks=m)
        # (3) per-query resident masks that differ, one None among them
        per = masks_of(n, nq, rng)
        el = np.stack([np.ones(n, dtype=bool) if p is None else p for p in per])
        handles = [None if p is None else ix.mask(p) for p in per]
        try:
            leg(ix, corpus, Q, k, what + ("per-query masks",), el, want, False, masks=handles)
        finally:
            for h in handles:
                if h is not None:
                    h.close()
        # (4) per-query raw allow words
        leg(ix, corpus, Q, k, what + ("raw allow",), el, want, False, allow=el)
        # (1) tombstones only: row 0, row n - 1 and a whole tile (where there is more than one)
        dead = np.zeros(n, dtype=bool)
        dead[[0, n - 1]] = True
        if n > 48:
            dead[32:48] = True
            dead[rng.integers(n, size=n // 50)] = True
        ix.tombstone_rows(np.flatnonzero(dead))
        leg(ix, corpus, Q, k, what + ("tombstones",), ~dead, want, True)
        # (5) tombstones and per-query masks
        leg(ix, corpus, Q, k, what + ("tombstones + raw allow",), el & ~dead, want, False, allow=el)


@pytest.mark.parametrize("dim,metric,nq", [(768, COS, 16), (384, EUC, 17), (64, COS, 3)], ids=["d768", "d384", "d64"])
def test_shared_mask_empties_whole_tiles(dim, metric, nq):
    """Leg 6: one mask that clears the first tile of every wave of block 0, the last tile, every tile of one wave's stride
    (a wave without any tile), and a run longer than one launch step; leg 8: a mask whose only eligible rows sit in the
    last, partial tile."""
    k = 10
    step = tsm.rows_per_step(dim)
    n = 3 * step + 77
    seed = SEED + 5000 + dim
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    n_tiles = (n + 15) // 16
    stride = step // 16   # tiles between two tiles of one wave (grid x waves)
    tile_ok = np.ones(n_tiles, dtype=bool)
    tile_ok[:WAVES] = False                 # the first tile of every wave of block 0
    tile_ok[n_tiles - 1] = False            # the last (partial) tile
    tile_ok[5::stride] = False              # wave 1 of block 1: no tile at all
    tile_ok[stride + 40: 2 * stride + 90] = False   # a run longer than one launch step
    holes = np.repeat(tile_ok, 16)[:n]
    with open_masked(dim, metric) as ix:
        ix.synth(n, seed)
        with ix.mask(holes) as m:
            leg(ix, corpus, Q, k, ("whole tiles", dim), holes, tsm.matrix_passes(nq), True, masks=m)
        tail = np.zeros(n, dtype=bool)
        tail[(n_tiles - 1) * 16:] = True   # 13 rows: the last tile alone
        with ix.mask(tail) as m:
            leg(ix, corpus, Q, k, ("last tile only", dim), tail, tsm.matrix_passes(nq), True, masks=m)


def test_few_rows_one_row_no_row():
    """Leg 7: masks that leave fewer than k rows, one row and none: counts and UINT64_MAX padding as under sketch_masked = 0
    and as the oracle's."""
    dim, metric, nq, k = 384, COS, 16, 10
    n = tsm.rows_per_step(dim) + 77
    seed = SEED + 6000
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    with open_masked(dim, metric) as ix:
        ix.synth(n, seed)
        for name, rows in (("seven rows", [3, 16, 17, 5000, n - 30, n - 2, n - 1]), ("one row", [n - 1]), ("no row", [])):
            el = np.zeros(n, dtype=bool)
            el[rows] = True
            seen = {}
            for opt in (1, 0):
                ix.set_option("sketch_masked", opt)
                with ix.mask(el) as m:
                    ix.reset_stats()
                    seen[opt] = ix.search_topk(Q, k, masks=m)
                    info = ix.sketch_masked_info()
                assert_answers_per_query(seen[opt], corpus, Q, k, el, (name, opt))
                assert (seen[opt][2] == len(rows)).all(), (name, opt, seen[opt][2])
                assert (info["launches"] >= 1 and info["skip_launches"] == info["launches"]) if opt else info["launches"] == 0, (name, opt, info)
            assert tsm.same(seen[1], seen[0]), name


def test_two_shards():
    """Leg 9: a handle of two shards on the one card, one resident mask for every query."""
    dim, metric, nq, k = 64, COS, 17, 10
    n = 2 * tsm.rows_per_step(dim) + 77
    seed = SEED + 7000
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    el = np.random.default_rng(71).random(n) < 0.3
    with open_masked(dim, metric, devices=[0, 0]) as ix:
        ix.load(corpus.packed)
        assert ix.sketch_info()["n_shards"] in (0, 2)
        with ix.mask(el) as m:
            leg(ix, corpus, Q, k, ("two shards",), el, tsm.matrix_passes(nq), True, masks=m)
        assert ix.sketch_info()["n_shards"] == 2


@pytest.mark.parametrize("dim,nq", [(768, 17), (768, 40), (384, 32), (64, 64)], ids=["wide17", "share40", "wide32", "share64"])
def test_wide_and_shared_forms(dim, nq):
    """Launches of 17 .. 32 (wide) and 33 .. 64 (shared) queries under sketch_wide = sketch_share = 2, with one mask for
    every query, per-query masks and tombstones: the passes of the unmasked forced plans (test_gpu_sketch_wide /
    test_gpu_sketch_share), the answers of sketch_masked = 0."""
    metric, k = COS, 10
    n = tsm.rows_per_step(dim) + 77
    seed = SEED + 8000 + dim
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    rng = np.random.default_rng(81 + nq)
    assert tsw.wide_serves(dim, n, k, 0) and tss.share_serves(dim, n, k, 0)
    want = tss.forced_passes(nq) if nq > 32 else tsw.forced_passes(nq)
    p = scan_masked_plan(dim, 8, nq, sketch_masked=1, sketch_wide=2, sketch_share=2)
    assert p["passes"] == want and (p["share"] if nq > 32 else p["wide"]), p
    with open_masked(dim, metric, sketch_wide=2, sketch_share=2) as ix:
        ix.synth(n, seed)
        shared = rng.random(n) < 0.4
        with ix.mask(shared) as m:
            leg_forced(ix, corpus, Q, k, ("forced", dim, nq, "one mask"), shared, want, True, masks=m)
        el = np.stack([rng.random(n) < (0.8, 0.3)[j % 2] for j in range(nq)])
        leg_forced(ix, corpus, Q, k, ("forced", dim, nq, "raw allow"), el, want, False, allow=el)
        dead = rng.random(n) < 0.02
        dead[[0, n - 1]] = True
        ix.tombstone_rows(np.flatnonzero(dead))
        leg_forced(ix, corpus, Q, k, ("forced", dim, nq, "tombstones"), ~dead, want, True)


def leg_forced(ix, corpus, Q, k, what, eligible, want_on, skip, **filt):
    """leg() for handles under forced wide / shared batches: with the option off a masked call splits into launches of the
    one-query kernel, one pass per query, whatever its batches."""
    return leg(ix, corpus, Q, k, what, eligible, want_on, skip, **filt)


def test_same_lists_whatever_the_order_of_arrival():
    """768 dimensions, 40 queries, one mask: three runs, then sketch_bulk = 1 and sketch_select = 1 -- identical answers."""
    dim, metric, nq, k = 768, COS, 40, 10
    n = tsm.rows_per_step(dim) + 77
    seed = SEED + 9000
    packed = tsm.synth_corpus(seed, n, dim)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    el = np.random.default_rng(91).random(n) < 0.5
    with open_masked(dim, metric) as ix:
        ix.synth(n, seed)
        with ix.mask(el) as m:
            runs = [ix.search_topk(Q, k, masks=m) for _ in range(3)]
            for name in ("sketch_bulk", "sketch_select"):
                ix.set_option(name, 1)
                ix.reset_stats()
                runs.append(ix.search_topk(Q, k, masks=m))
                assert ix.sketch_masked_info()["launches"] >= 1, name
                ix.set_option(name, 0)
        for r in runs[1:]:
            assert tsm.same(runs[0], r)
        tsm.assert_answers(runs[0], packed, dim, metric, Q, k, el, ("determinism",))


def test_collection_where_and_removed_documents():
    """Leg 10: a Collection with an indexed field and removed documents, SearchBatch of 17 queries with Where: the same
    answers with and without the option, and masked matrix launches with it."""
    dim, n, nq, k = 64, 6000, 17, 10
    V = orc.synth_vectors(SEED + 9500, 0, n, dim)
    q = orc.synth_vectors(SEED + 9501, 0, nq, dim)
    c = Collection(CollectionOptions(Name="masked", DistanceMethod=1, DimensionCount=dim, Quantization=32), devices=[0])
    try:
        c.AddDocuments(range(n), V, [('{"price": %d}' % (i % 10)).encode() for i in range(n)])
        c.IndexField("price", "number")
        for id_ in (0, 17, 4000, n - 1):
            c.removeDocument(id_)
        for name, value in (("sketch", 1), ("sketch_min_rows", 1), ("multi_query", 0)):
            c._index.set_option(name, value)
        args = [SearchArgs(Vector=q[i], K=k, Where=Field("price") < 5) for i in range(nq)]
        seen = {}
        for opt in (0, 1):
            c._index.set_option("sketch_masked", opt)
            c._index.reset_stats()
            got = c.SearchBatch(args)
            seen[opt] = [[(r.ID, r.Distance) for r in g.Results] for g in got]
            info = c._index.sketch_masked_info()
            assert (info["launches"] >= 1) == bool(opt), (opt, info)
        assert seen[0] == seen[1]
        assert all(len(x) == k and all(id_ % 10 < 5 and id_ not in (0, 17, 4000, n - 1) for id_, _ in x) for x in seen[1])
    finally:
        c.Close()
