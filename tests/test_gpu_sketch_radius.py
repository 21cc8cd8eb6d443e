"""Radius searches through the 8-bit sketch (option sketch_radius; scan_radius.cpp, kernels_scan_mx.hip's collect form).

Handles are opened like test_gpu_sketch_matrix.open_sketched (sketch = 1, sketch_min_rows = 1, the certificate trace on)
plus sketch_radius = 1.  Radii come from the oracle: per query the midpoint between its m-th and (m + 1)-th float64
distance, m in (0, 1, 25, 300) -- no predicate sits on a rounding edge, and the zero-hit case exists.  Every case
asserts: the hits equal the oracle's radius answer (rows in order, distances bit-equal); K_s, C_s, T and S_r hold on
the trace (cert_check); sketch_radius_queries + sketch_radius_fallbacks == the call's query count.  Pass counts are read
off szg_stats.scan_bytes in sketch rows (dim bytes each), exactly when the sketch settled every query: a query handed
over adds a sweep of the float32 rows, 4 such units.

How a call with one sweep per query splits into launches: test_gpu_sketch_matrix.launch_sizes (the sketch pre-pass's
plan, which SketchRadiusCall::plan follows)."""
import numpy as np
import pytest

import oracle as orc
import test_gpu_sketch_matrix as tsm
from syzgydb_amd import Collection, CollectionOptions, Cosine, SearchArgs, _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import scan_collect_plan

pytestmark = pytest.mark.gpu

SEED = 0x53595A470000D000
EUC, COS = tsm.EUC, tsm.COS
MID = tsm.MID
POOL = tsm.POOL
DEFAULT_TUNABLES = tsm.DEFAULT_TUNABLES
MS = (0, 1, 25, 300)


def open_radius(dim, metric, devices=None, **options):
    return tsm.open_sketched(dim, metric, devices=devices, **dict({"sketch_radius": 1, "radius_mq": 0}, **options))


def all_dists(corpus, Q):
    return np.stack(list(POOL.map(lambda q: orc.all_distances(corpus.packed, corpus.dim, 32, corpus.metric, q), Q)))


def radius_at(d, m, eligible=None):
    """The midpoint between the m-th and the (m + 1)-th smallest distance (m = 0: between 0 and the smallest)."""
    s = np.sort(d[np.isfinite(d) & (True if eligible is None else eligible)])
    m = min(m, s.size - 1)
    r = float(s[m] / 2 if m == 0 else (s[m - 1] + s[m]) / 2)
    assert r > 0 and (m == 0 or s[m - 1] < r) and r < s[m], ("the radius sits on an edge", m, s[:m + 1][-2:])
    return r


def radii_for(dists, ms=MS, eligible=None):
    return np.array([radius_at(d, ms[i % len(ms)], eligible) for i, d in enumerate(dists)])


def oracle_hits(corpus, Q, radii, eligible):
    """The oracle's radius answers, (rows, distances) per query.  eligible: None, bool[n] for all or bool[nq, n]."""
    allow = [None] * len(Q) if eligible is None else np.broadcast_to(eligible, (len(Q), eligible.shape[-1])).astype(np.uint8)
    return list(POOL.map(lambda a: orc.search_exact(corpus.packed, corpus.dim, 32, corpus.metric, a[0], radius=float(a[1]),
                                                    allow=a[2])[:2], zip(Q, radii, allow)))


def assert_same_as(got, want, what):
    for qi, (w_rows, w_dist) in enumerate(want):
        g_rows, g_dist = got[qi]
        assert [int(x) for x in g_rows] == [int(x) for x in w_rows], ("rows differ", what, qi, len(g_rows), len(w_rows))
        assert (np.asarray(g_dist) == w_dist).all(), ("distances not bit-equal", what, qi)


def assert_hits(got, corpus, Q, radii, eligible, what):
    assert_same_as(got, oracle_hits(corpus, Q, radii, eligible), what)


def same_hits(a, b):
    return len(a) == len(b) and all((x[0] == y[0]).all() and (x[1] == y[1]).all() and len(x[0]) == len(y[0]) for x, y in zip(a, b))


def checked_call(ix, corpus, Q, radii, what, dists, eligible=None, lone=False, **filt):
    """One radius call (lone: one szg_search_radius per query) through the sketch: the hits against the oracle, the
    chain on the trace, the counters.  -> (hits, stats, records of the sketch-radius pass)"""
    Q = np.atleast_2d(Q)
    nq = Q.shape[0]
    ix.reset_stats()
    ix.certificates()
    if lone:
        got, recs_all = [], []
        for qi in range(nq):
            got.append(ix.search_radius(Q[qi], float(radii[qi])))
            recs, ents, dropped = ix.certificates()
            recs_all.append((recs, ents, dropped))
    else:
        got = ix.search_radius_batch(Q, radii, **filt)
        recs_all = [ix.certificates()]
    st = ix.stats()
    assert st["sketch_radius_queries"] + st["sketch_radius_fallbacks"] == nq, (what, st)
    assert_hits(got, corpus, Q, radii, eligible, what)
    info = ix.sketch_info()
    assert info["in_sync"] == 1, (what, info)
    sk_corpus = cc.Corpus(ix.sketch_rows()[0], corpus.dim, 8, corpus.metric)
    n_rec = 0
    for i, (recs, ents, dropped) in enumerate(recs_all):
        qs = slice(i, i + 1) if lone else slice(None)
        el = eligible if eligible is None or eligible.ndim == 1 else eligible[qs]
        s = cc.check(corpus, Q[qs], recs, ents, dropped, eligible=el, dists=dists[qs], what=what,
                     sketch=(sk_corpus, info["gscale"], info["exc_rows"]), radii=radii[qs])
        own = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH_RADIUS]
        n_rec += len(own)
        assert len(set(int(x) for x in own["query"])) == len(own), ("one record per query", what)
    assert n_rec == st["sketch_radius_queries"], ("one sketch-radius record per settled query", what, n_rec, st)
    return got, st, recs_all


def assert_passes(st, n, dim, nq, want, what):
    """`want` passes of the sketch; exact when every query was settled (a hand-over adds 4 per float32 sweep)."""
    if not DEFAULT_TUNABLES:
        return
    p = tsm.sketch_passes(st, n, dim, what)
    print(what, "passes (sketch rows)", p, "expected", want, "settled", st["sketch_radius_queries"], "of", nq)
    assert p % 4 == want % 4 and p >= want, (what, p, want, st)
    if st["sketch_radius_fallbacks"] == 0:
        assert p == want, (what, p, want)


# ---- 1. lone calls: the one-query collect kernel on the sketch ------------------------------------------------------------

@pytest.mark.parametrize("metric", (COS, EUC), ids=["cos", "euc"])
@pytest.mark.parametrize("dim", (64, 384))
def test_lone_calls(dim, metric):
    n, nq = 20000, 8
    seed = SEED + dim + metric
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    dists = all_dists(corpus, Q)
    radii = radii_for(dists)
    what = ("lone", dim, MID[metric])
    with open_radius(dim, metric, radius_mq=1) as ix:   # (a lone call takes a sweep of its own whatever radius_mq says)
        ix.synth(n, seed)
        got, st, _ = checked_call(ix, corpus, Q, radii, what, dists, lone=True)
        # m <= 25 of 20 000 rows: a few dozen candidates, far below the first buffer's 1 024 entries
        assert st["sketch_radius_queries"] >= 6, (what, st)
        assert st["scan_launches"] >= nq
        if st["sketch_radius_fallbacks"] == 0 and DEFAULT_TUNABLES:
            assert st["scan_bytes"] == nq * n * dim, ("a quarter of the bytes: one sketch row per row and query", what, st)
        assert_passes(st, n, dim, nq, nq, what)
        assert ix.stats()["sketch_queries"] + ix.stats()["sketch_fallbacks"] == 0   # (no top-k went by)
        ix.set_option("sketch_radius", 0)
        ix.reset_stats()
        got0 = [ix.search_radius(Q[i], float(radii[i])) for i in range(nq)]
        st0 = ix.stats()
        assert same_hits(got, got0)
        assert st0["sketch_radius_queries"] + st0["sketch_radius_fallbacks"] == 0 and st0["scan_bytes"] == nq * n * dim * 4, st0


# ---- 2. the matrix collect lattice ------------------------------------------------------------------------------------------

LATTICE = [(dim, rows, metric) for dim in (64, 192, 384) for rows in (15, 16, 17, "s1") for metric in (COS, EUC)]
LATTICE += [(768, "s1", COS)]


def lattice_id(c):
    return "d%d-n%s-%s" % (c[0], c[1], MID[c[2]])


@pytest.mark.parametrize("case", LATTICE, ids=[lattice_id(c) for c in LATTICE])
def test_matrix_collect_lattice(case):
    dim, rows, metric = case
    n = tsm.n_rows_of(dim, rows)
    seed = SEED + dim * 100 + (n % 1000)
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Qall = orc.synth_vectors(seed + 1, 0, 40, dim) * 0.7
    dall = all_dists(corpus, Qall)
    rall = radii_for(dall)
    with open_radius(dim, metric) as ix:
        ix.synth(n, seed)
        assert (ix.read_rows(n - 1, 1) == corpus.packed[n - 1:]).all()
        for nq in (3, 16, 17, 40):
            what = ("lattice", lattice_id(case), "rows", n, "queries", nq)
            Q, dists, radii = Qall[:nq], dall[:nq], rall[:nq]
            for n_l in tsm.launch_sizes(nq):   # the plan: every launch of this call is one the collect form takes
                assert scan_collect_plan(dim, 8, n_l)["serves"]
            ix.set_option("sketch_matrix", 0)
            got, st, _ = checked_call(ix, corpus, Q, radii, what, dists)
            assert_passes(st, n, dim, nq, tsm.matrix_passes(nq), what)
            ix.set_option("sketch_matrix", 1)   # one-query collect sweeps of the sketch
            got1, st1, _ = checked_call(ix, corpus, Q, radii, what + ("sketch_matrix = 1",), dists)
            assert same_hits(got, got1), ("hits differ from the one-query collect kernel's", what)
            assert_passes(st1, n, dim, nq, nq, what + ("sketch_matrix = 1",))
        ix.set_option("sketch_matrix", 0)
        for name, value in (("sketch_radius", 0), ("sketch", 0)):
            ix.set_option(name, value)
            ix.reset_stats()
            got0 = ix.search_radius_batch(Qall, rall)
            assert same_hits(got0[:nq], got) and ix.stats()["sketch_radius_queries"] == 0, (name, case)


# ---- 3. the wide form -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", (384, 768))
def test_wide_form(dim):
    metric = COS
    n = tsm.rows_per_step(dim) + 77
    seed = SEED + 7000 + dim
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Qall = orc.synth_vectors(seed + 1, 0, 40, dim) * 0.7
    dall = all_dists(corpus, Qall)
    rall = radii_for(dall)
    assert scan_collect_plan(dim, 8, 32, sketch_wide=2)["wide"]
    with open_radius(dim, metric, sketch_wide=2) as ix:
        ix.synth(n, seed)
        for nq in (33, 40):
            what = ("wide", dim, nq)
            ix.set_option("sketch_wide", 2)
            got, st, _ = checked_call(ix, corpus, Qall[:nq], rall[:nq], what, dall[:nq])
            assert_passes(st, n, dim, nq, 2, what)   # batches of 32 and the rest: one pass per launch of up to 32
            ix.set_option("sketch_wide", 1)
            got1, st1, _ = checked_call(ix, corpus, Qall[:nq], rall[:nq], what + ("sketch_wide = 1",), dall[:nq])
            assert same_hits(got, got1), what
            assert_passes(st1, n, dim, nq, tsm.matrix_passes(nq), what + ("sketch_wide = 1",))


# ---- 4. a crowded tile --------------------------------------------------------------------------------------------------------

def test_crowded_tile():
    """40 rows within the radius inside one wave's first tiles, 16 near-copies of the query: many hit lanes per 16-lane
    slice and several slots per tile -- the rank and base arithmetic of the collect form.  Counts and entries exact."""
    dim, n, nq = 64, 20000, 16
    V, q = tsm.crowded_block(1500, n, dim)
    corpus = cc.Corpus(orc.encode_rows(V, 32), dim, 32, COS)
    Q = np.stack([q * (1.0 + 0.25 * i) + 1e-5 * i * np.arange(dim) / dim for i in range(nq)])
    dists = all_dists(corpus, Q)
    radii = radii_for(dists, ms=(40,))
    with open_radius(dim, COS) as ix:
        ix.load(corpus.packed)
        got, st, recs_all = checked_call(ix, corpus, Q, radii, ("crowded",), dists)
        assert st["sketch_radius_fallbacks"] == 0, st
        assert_passes(st, n, dim, nq, tsm.matrix_passes(nq), ("crowded",))
        recs, ents, _ = recs_all[0]
        for rec in recs:
            e = ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]
            rows = sorted(int(x) for x in e["row"])
            assert len(set(rows)) == len(rows), ("an entry twice", int(rec["query"]))
            assert set(range(40)) <= set(rows), ("a planted row is not among the entries", int(rec["query"]))
        for qi in range(nq):
            assert sorted(int(x) for x in got[qi][0]) == list(range(40)), qi
        ix.set_option("sketch_matrix", 1)
        got1, _, recs_1 = checked_call(ix, corpus, Q, radii, ("crowded", "sketch_matrix = 1"), dists)
        assert same_hits(got, got1)
        # the widened radius ends far below the random rows' distances: exactly the planted rows, under both kernels
        for rec in list(recs) + list(recs_1[0][0]):
            assert int(rec["n_entries"]) == 40, (int(rec["query"]), int(rec["n_entries"]))


# ---- 5. the last tile ---------------------------------------------------------------------------------------------------------

def test_last_tile_and_idle_columns_never_appear():
    """17 rows in a handle that held 32 whose rows 17 .. 31 lie closest to every query, a call of 17 queries (launches of
    13 and 4: idle columns in both) and a take-all radius just under the hand-over rule: exactly the 17 rows."""
    dim, nq = 64, 17
    rng = np.random.default_rng(4200)
    Q = rng.standard_normal((nq, dim))
    V = rng.standard_normal((32, dim))
    V[17:] = Q.mean(axis=0) * (1.0 + 0.01 * np.arange(15))[:, None]
    packed = orc.encode_rows(V, 32)
    with open_radius(dim, COS) as ix:
        ix.load(packed)
        ix.search_radius_batch(Q, 0.3)   # (the sketch of the 32 rows is built)
        ix.load(packed[:17])
        ix.search_radius_batch(Q[:3], 0.3)
        slack = cc.sketch_slack(ix.sketch_info()["max_ang"], 0.0, dim)
        corpus = cc.Corpus(packed[:17], dim, 32, COS)
        dists = all_dists(corpus, Q)
        radii = np.full(nq, 0.999 - slack)   # D = R (1 + 1e-9) + slack just under 1
        got, st, _ = checked_call(ix, corpus, Q, radii, ("last tile",), dists)
        assert st["sketch_radius_fallbacks"] == 0, st
        for qi in range(nq):
            assert sorted(int(x) for x in got[qi][0]) == list(range(17)), (qi, got[qi][0])
        assert_passes(st, 17, dim, nq, 2, ("last tile",))


# ---- 6. steps aside -----------------------------------------------------------------------------------------------------------

def test_masked_and_tombstoned_launches_keep_the_one_query_kernel():
    dim, metric, nq = 384, COS, 16
    n = tsm.rows_per_step(dim) + 77
    seed = SEED + 9100
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    dists = all_dists(corpus, Q)
    allow = np.arange(n) % 5 != 2
    with open_radius(dim, metric) as ix:
        ix.synth(n, seed)
        radii = radii_for(dists, eligible=allow)
        got, st, _ = checked_call(ix, corpus, Q, radii, ("filter",), dists, eligible=allow, allow=np.stack([allow] * nq))
        assert_passes(st, n, dim, nq, nq, ("filter",))
        with ix.mask_rows(np.flatnonzero(allow)) as mask:
            got_m, st_m, _ = checked_call(ix, corpus, Q, radii, ("mask handle",), dists, eligible=allow, masks=mask)
        assert same_hits(got, got_m)
        assert_passes(st_m, n, dim, nq, nq, ("mask handle",))
        dead = np.zeros(n, dtype=bool)
        dead[[0, 5, n // 2, n - 1]] = True
        dead[[int(got[1][0][0]), int(got[2][0][0])]] = True   # two rows that were hits
        ix.tombstone_rows(np.flatnonzero(dead))
        radii = radii_for(dists, eligible=~dead)
        got_d, st_d, _ = checked_call(ix, corpus, Q, radii, ("tombstones",), dists, eligible=~dead)
        assert_passes(st_d, n, dim, nq, nq, ("tombstones",))


def test_hand_overs():
    """A zero cosine query, R = 0.9999 (D >= 1), a NaN element and a radius of inf: handed to the float32 sweep, counted,
    answered as with sketch_radius = 0."""
    dim, n = 64, 3000
    seed = SEED + 9200
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, COS)
    Q = orc.synth_vectors(seed + 1, 0, 6, dim) * 0.7
    Q[0] = 0.0
    Q[2, 7] = np.nan
    dists = all_dists(corpus, Q[4:])
    radii = np.array([0.4, 0.9999, 0.45, np.inf, radius_at(dists[0], 25), radius_at(dists[1], 1)])
    for metric in (COS, EUC):
        with open_radius(dim, metric) as ix:
            ix.synth(n, seed)
            ix.reset_stats()
            got = ix.search_radius_batch(Q, radii)
            st = ix.stats()
            want_fb = 4 if metric == COS else 2   # (Euclid: a zero query and R = 0.9999 are ordinary)
            assert st["sketch_radius_fallbacks"] >= want_fb and st["sketch_radius_queries"] + st["sketch_radius_fallbacks"] == 6, st
            if DEFAULT_TUNABLES and metric == COS:
                assert st["sketch_radius_fallbacks"] == 4 and st["sketch_radius_queries"] == 2, st
            lone = ix.search_radius(Q[0], 0.4)
            ix.set_option("sketch_radius", 0)
            got0 = ix.search_radius_batch(Q, radii)
            assert same_hits(got, got0), metric
            assert same_hits([lone], [ix.search_radius(Q[0], 0.4)])
            assert len(got[3][0]) == n and len(got[2][0]) == 0, (len(got[3][0]), len(got[2][0]))
    assert_hits(got[4:], corpus.with_metric(EUC), Q[4:], radii[4:], None, ("hand-overs: the ordinary queries",))


# ---- 7. overflow --------------------------------------------------------------------------------------------------------------

def test_overflow_then_a_small_radius():
    dim, n = 64, 20000
    seed = SEED + 9300
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, COS)
    Q = orc.synth_vectors(seed + 1, 0, 2, dim) * 0.7
    dists = all_dists(corpus, Q)
    with open_radius(dim, COS) as ix:
        ix.synth(n, seed)
        big = np.array([radius_at(dists[0], n // 2)])
        got, st, _ = checked_call(ix, corpus, Q[:1], big, ("overflow",), dists[:1], lone=True)
        assert len(got[0][0]) == n // 2
        small = np.array([radius_at(dists[1], 25)])
        got, st, _ = checked_call(ix, corpus, Q[1:], small, ("after the overflow",), dists[1:], lone=True)
        assert st["sketch_radius_queries"] == 1 and st["sketch_radius_fallbacks"] == 0, st
        assert len(got[0][0]) == 25


def test_hit_lists_larger_than_one_block_travel_list_by_list():
    """Four queries of 30 000 hits each in 60 000 rows.  The first call overflows the fresh contexts' 1 024-entry buffers
    and hands all four over; the contexts have then seen at least 30 000 candidates per query, so the second call's
    buffers hold 65 536 entries or more per query -- more than there are rows: no overflow -- and its block, 4 x cap x 16
    bytes >= 4 MiB, is beyond max(2 MiB, 4 x 64 KiB): the hits come back list by list, each longer than the device sorts
    (kSortHitsMax = 2 048), so the host does.  The trace is off: records of this size need not fit it."""
    dim, n, nq = 64, 60000, 4
    seed = SEED + 9350
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, COS)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    dists = all_dists(corpus, Q)
    big = np.array([radius_at(d, 30000) for d in dists])
    want = oracle_hits(corpus, Q, big, None)
    assert all(len(w[0]) == 30000 for w in want)
    with open_radius(dim, COS) as ix:
        ix.trace_certificates(False)
        ix.synth(n, seed)
        for call in ("first", "second"):
            ix.reset_stats()
            got = ix.search_radius_batch(Q, big, capacity=nq * 30000)   # (room for all: the call is made once)
            st = ix.stats()
            assert_same_as(got, want, (call, "call"))
            assert st["sketch_radius_queries"] + st["sketch_radius_fallbacks"] == nq, (call, st)
            if DEFAULT_TUNABLES:
                settled = 0 if call == "first" else nq
                assert (st["sketch_radius_queries"], st["sketch_radius_fallbacks"]) == (settled, nq - settled), (call, st)
        small = np.array([radius_at(d, 25) for d in dists])
        ix.reset_stats()
        got = ix.search_radius_batch(Q, small)
        st = ix.stats()
        assert_hits(got, corpus, Q, small, None, ("third call",))
        assert st["sketch_radius_queries"] + st["sketch_radius_fallbacks"] == nq, st
        assert all(len(g[0]) == 25 for g in got)


# ---- 8. rows without a usable sketch ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", (COS, EUC), ids=["cos", "euc"])
def test_rows_without_a_sketch(metric):
    dim, n, nq = 64, 600, 5
    rng = np.random.default_rng(4300 + metric)
    q = rng.standard_normal(dim)
    V = q[None, :] + 0.3 * rng.standard_normal((n, dim))   # close rows
    V = V.astype(np.float32).astype(np.float64)
    zero, inf, nan = 100, 200, 300
    V[zero] = 0.0
    V[inf, 3] = np.inf
    V[nan, 9] = np.nan
    corpus = cc.Corpus(orc.encode_rows(V, 32), dim, 32, metric)
    Q = np.stack([q * (1.0 + 0.1 * i) for i in range(nq)])
    dists = all_dists(corpus, Q)
    radii = np.array([np.sort(d[np.isfinite(d)])[n // 2] * 1.0000001 for d in dists])
    with open_radius(dim, metric) as ix:
        ix.load(corpus.packed)
        got, st, recs_all = checked_call(ix, corpus, Q, radii, ("unsketched rows", MID[metric]), dists)
        exc = set(int(x) for x in ix.sketch_info()["exc_rows"])
        assert {inf, nan} <= exc and (metric != COS or zero in exc), exc
        recs, ents, _ = recs_all[0]
        own = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH_RADIUS]
        assert len(own) + st["sketch_radius_fallbacks"] == nq
        for rec in own:
            e = ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]
            no_key = set(int(x) for x in e["row"][(e["flags"] & _lib.SZG_CERT_ENTRY_NO_KEY) != 0])
            assert no_key == exc, (int(rec["query"]), no_key, exc)
        for qi in range(nq):
            rows = set(int(x) for x in got[qi][0])
            assert nan not in rows
            for r in (zero, inf):   # (the oracle decides; the answer above was compared with it row by row)
                assert (r in rows) == bool(dists[qi, r] <= radii[qi]), (qi, r)
        lone = [ix.search_radius(Q[i], float(radii[i])) for i in range(nq)]
        assert same_hits(lone, got)


def test_two_shards():
    """A handle of two shards (both on device 0), a row without a usable sketch in each: every shard stages its own head,
    and a query's hits come as one list per shard (never presorted).  Then the same call with a mask on three of the
    twelve queries -- launches of the one-query kernel, heads that differ from query to query."""
    dim, n, nq = 64, 9000, 12
    rng = np.random.default_rng(4350)
    V = rng.standard_normal((n, dim)).astype(np.float32).astype(np.float64)
    exc = {1000, 8000}
    V[1000, 3] = np.inf
    V[8000, 5] = np.inf
    corpus = cc.Corpus(orc.encode_rows(V, 32), dim, 32, COS)
    Q = rng.standard_normal((nq, dim))
    dists = all_dists(corpus, Q)
    radii = radii_for(dists)
    allow = np.arange(n) % 3 != 1   # (row 1000 is out, row 8000 is in)
    masked = (2, 5, 9)
    eligible = np.ones((nq, n), dtype=bool)
    eligible[list(masked)] = allow
    with open_radius(dim, COS, devices=[0, 0]) as ix:
        ix.load(corpus.packed)
        got, st, recs_all = checked_call(ix, corpus, Q, radii, ("two shards",), dists)
        info = ix.sketch_info()
        assert info["n_shards"] == 2 and set(int(x) for x in info["exc_rows"]) == exc, info
        recs, ents, _ = recs_all[0]
        for rec in recs[recs["pass_"] == _lib.SZG_CERT_SKETCH_RADIUS]:
            e = ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]
            no_key = set(int(x) for x in e["row"][(e["flags"] & _lib.SZG_CERT_ENTRY_NO_KEY) != 0])
            assert no_key == exc, ("one staged row per shard", int(rec["query"]), no_key)
        if DEFAULT_TUNABLES:
            assert st["sketch_radius_fallbacks"] == 0, st
        assert max(len(g[0]) for g in got) >= 300 and min(len(g[0]) for g in got) == 0
        with ix.mask(allow) as mask:
            handles = [mask if i in masked else None for i in range(nq)]
            got_m, st_m, _ = checked_call(ix, corpus, Q, radii, ("two shards, masks",), dists, eligible=eligible, masks=handles)
            assert_passes(st_m, n, dim, nq, nq, ("two shards, masks",))
            ix.set_option("sketch_radius", 0)
            ix.reset_stats()
            got0, got0_m = ix.search_radius_batch(Q, radii), ix.search_radius_batch(Q, radii, masks=handles)
            assert ix.stats()["sketch_radius_queries"] + ix.stats()["sketch_radius_fallbacks"] == 0
        assert same_hits(got, got0) and same_hits(got_m, got0_m)


# ---- 9. mutations -------------------------------------------------------------------------------------------------------------

def test_mutations_and_the_collection_mirror():
    dim, n, metric = 64, 5000, COS
    rng = np.random.default_rng(4400)
    V = rng.standard_normal((n + 50, dim)).astype(np.float32).astype(np.float64)
    Q = rng.standard_normal((4, dim))
    with open_radius(dim, metric) as ix:
        ix.load(orc.encode_rows(V[:n], 32))
        cur = V[:n].copy()
        alive = np.ones(n, dtype=bool)

        def step(what):
            corpus = cc.Corpus(orc.encode_rows(cur, 32), dim, 32, metric)
            dists = all_dists(corpus, Q)
            radii = radii_for(dists, ms=(25, 1, 300, 0), eligible=alive)
            got, st, _ = checked_call(ix, corpus, Q, radii, (what,), dists, eligible=alive)
            assert st["sketch_radius_queries"] >= 3, (what, st)
            lone = ix.search_radius(Q[0], float(radii[0]))
            assert same_hits([lone], got[:1])
            return got

        got = step("loaded")
        ix.append(orc.encode_rows(V[n:], 32))
        cur = V.copy()
        alive = np.ones(n + 50, dtype=bool)
        got = step("appended")
        hit = int(got[0][0][0])
        cur[hit] = -Q[0]   # a hit row moved far away
        ix.overwrite_rows([hit], orc.encode_rows(cur[hit:hit + 1], 32))
        got = step("overwritten")
        assert hit not in set(int(x) for x in got[0][0])
        hit = int(got[0][0][0])
        ix.tombstone_rows([hit])
        alive[hit] = False
        got = step("tombstoned")
        assert hit not in set(int(x) for x in got[0][0])

    ids = list(range(1, n + 1))
    a = Collection(CollectionOptions(Name="a", DistanceMethod=Cosine, DimensionCount=dim, Quantization=32), sketch=False)
    b = Collection(CollectionOptions(Name="b", DistanceMethod=Cosine, DimensionCount=dim, Quantization=32), sketch=True)
    for c in (a, b):
        c.AddDocuments(ids, V[:n], [b"m%d" % i for i in ids])
    d0 = np.sort(orc.all_distances(orc.encode_rows(V[:n], 32), dim, 32, COS, Q[1]))
    for r in ((d0[9] + d0[10]) / 2, d0[0] / 2):
        ra = a.Search(SearchArgs(Vector=Q[1], Radius=float(r), Precision="exact"))
        rb = b.Search(SearchArgs(Vector=Q[1], Radius=float(r), Precision="exact"))
        assert [(x.ID, x.Distance, x.Metadata) for x in ra.Results] == [(x.ID, x.Distance, x.Metadata) for x in rb.Results]
    assert len(ra.Results) == 0
    assert b._index.stats()["sketch_radius_queries"] >= 2 and a._index.stats()["sketch_radius_queries"] == 0
    a.Close()
    b.Close()


# ---- 10. default off ----------------------------------------------------------------------------------------------------------

def test_default_off():
    dim, n = 64, 20000
    seed = SEED + 9400
    q = orc.synth_vectors(seed + 1, 0, 1, dim)[0]
    with tsm.open_sketched(dim, COS) as ix:   # sketch = 1, but no sketch_radius
        ix.synth(n, seed)
        ix.reset_stats()
        ix.search_radius(q, 0.3)
        st = ix.stats()
        assert st["scan_bytes"] == n * dim * 4, st   # today's sweep of the float32 rows
        ix.search_radius_batch(np.stack([q, q * 2]), 0.3)
        st = ix.stats()
        assert st["sketch_radius_queries"] == 0 and st["sketch_radius_fallbacks"] == 0, st
        assert ix.sketch_info()["exists"] == 0   # no radius search builds a sketch index under the default
