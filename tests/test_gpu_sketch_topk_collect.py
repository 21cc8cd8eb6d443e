"""Top-k searches of large k through the 8-bit sketch (option sketch_topk_collect; scan_sketch_topk.cpp SketchTopkCall,
kernels_sample_mx.hip, sample_plan.h): a sample pass bounds the k-th distance, a collect sweep at that radius contains the
answer.

Handles are opened like test_gpu_sketch_matrix.open_sketched (sketch = 1, sketch_min_rows = 1, multi_query = 0, the
certificate trace on) plus sketch_topk_collect = 1.  Every call asserts: ids and float64 distances == the oracle's and ==
the same handle's answers with the option at 0; cert_check holds on every record (K_s, C_s, T, P, R, S_k, F);
sketch_topk_stats' queries + fallbacks == the call's queries; and, under default tunables, szg_stats.scan_bytes is what the
plan says: per sample launch the sample's rows, per collect launch one pass over the sketch rows (dim bytes per row), four
such passes per query handed to the float32 sweep.

So that no case passes by handing everything over: wherever nothing degenerate is planted the test first counts, from the
oracle's distances and the record's D, the rows within D + slack -- every row the sweep can collect lies there -- checks
that they are fewer than the plan's starting capacity, and then asserts fallbacks == 0.

How a call splits: up to 32 queries are ONE batch (from 8 on its collect sweeps go in two parts, the last min(4, n / 2)
apart); longer calls go in batches of 4, 16, 16, ..., 4.  A sample launch holds up to 16 queries of a batch; a collect
launch of 3 queries or more without masks is one pass, any other one pass per query.

The largest ratio of a settled query's candidates to k x stride seen over this file is printed per case (-s shows it) and
recorded in profiles/sketch_topk_collect.txt."""
import numpy as np
import pytest

import oracle as orc
import test_gpu_sketch_matrix as tsm
from syzgydb_amd import ScanIndex, _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import sample_plan

pytestmark = pytest.mark.gpu

SEED = 0x53595A470000E000
EUC, COS = tsm.EUC, tsm.COS
MID = tsm.MID
POOL = tsm.POOL
DEFAULT_TUNABLES = tsm.DEFAULT_TUNABLES
PASS = _lib.SZG_CERT_SKETCH_TOPK_COLLECT
RATIO = {"max": 0.0}


def open_tc(dim, metric, devices=None, **options):
    return tsm.open_sketched(dim, metric, devices=devices, **dict({"sketch_topk_collect": 1}, **options))


def all_dists(corpus, Q):
    return np.stack(list(POOL.map(lambda q: orc.all_distances(corpus.packed, corpus.dim, corpus.bits, corpus.metric, q), Q)))


def oracle_topk(corpus, Q, k, eligible):
    nq = len(Q)
    allow = [None] * nq if eligible is None else np.broadcast_to(eligible, (nq, eligible.shape[-1])).astype(np.uint8)
    return list(POOL.map(lambda a: orc.search_exact(corpus.packed, corpus.dim, corpus.bits, corpus.metric, a[0], k=k,
                                                    allow=a[1])[:2], zip(Q, allow)))


def assert_answers(got, want, what, rows_too=True):
    r, d, cnt = got
    for qi, (w_rows, w_dist) in enumerate(want):
        assert cnt[qi] == len(w_rows), ("result counts differ", what, qi, cnt[qi], len(w_rows))
        g = d[qi, : cnt[qi]]
        assert ((g == w_dist) | (np.isnan(g) & np.isnan(w_dist))).all(), ("distances not bit-equal", what, qi)
        if rows_too:
            assert [int(x) for x in r[qi, : cnt[qi]]] == [int(x) for x in w_rows], ("rows differ", what, qi)


def batch_sizes(nq):
    if nq <= 32:
        return [nq]
    parts, q0 = [], 0
    while q0 < nq:
        left = nq - q0
        n = min(16, left)
        if left > 4:
            n = min(n, 4) if q0 == 0 else (left - 4 if left <= 20 else n)
        parts.append(n)
        q0 += n
    return parts


def expected_bytes(shard_rows, dim, nq, k, masked):
    """szg_stats.scan_bytes of a call every query of which is settled, by the plan."""
    total = 0
    for n in shard_rows:
        sp = sample_plan(n, k, 1, dim)
        total += sum(-(-b // 16) for b in batch_sizes(nq)) * sp["sample_rows"] * dim
        if masked:
            passes = nq
        else:
            passes = sum(1 if m >= 3 else m for m in tsm.launch_sizes(nq))
        total += passes * n * dim
    return total


def checked_call(ix, corpus, Q, k, what, dists, eligible=None, plain=True, rows_too=True, shard_rows=None, **filt):
    """One top-k call with the option on: the answers, the chain on the trace, the counters, the pass count.  plain: nothing
    degenerate is planted -- no query may be handed over.  -> (answers, sketch_topk_stats, records of the pass)"""
    Q = np.atleast_2d(Q)
    nq, n, dim = Q.shape[0], corpus.n, corpus.dim
    ix.reset_stats()
    ix.certificates()
    got = ix.search_topk(Q, k, **filt)
    recs, ents, dropped = ix.certificates()
    st, ts = ix.stats(), ix.sketch_topk_stats()
    assert ts["queries"] + ts["fallbacks"] == nq, (what, ts)
    assert_answers(got, oracle_topk(corpus, Q, k, eligible), what, rows_too)
    info = ix.sketch_info()
    assert info["in_sync"] == 1, (what, info)
    sk_corpus = cc.Corpus(ix.sketch_rows()[0], dim, 8, corpus.metric)
    cc.check(corpus, Q, recs, ents, dropped, eligible=eligible, dists=dists, what=what,
             sketch=(sk_corpus, info["gscale"], info["exc_rows"]))
    own = recs[recs["pass_"] == PASS]
    assert sorted(int(x) for x in own["query"]) == list(range(nq)), ("one record per query", what)
    assert int((own["certified"] == 1).sum()) == ts["queries"], (what, ts)
    # the same handle with the option at 0
    ix.set_option("sketch_topk_collect", 0)
    ix.reset_stats()
    got0 = ix.search_topk(Q, k, **filt)
    ts0 = ix.sketch_topk_stats()
    ix.set_option("sketch_topk_collect", 1)
    assert ts0 == dict.fromkeys(ts0, 0), ("the option at 0 counts nothing", what, ts0)
    assert (got[2] == got0[2]).all() and (got[1] == got0[1])[~np.isnan(got[1])].all(), ("differs from the option at 0", what)
    if rows_too:
        assert (got[0] == got0[0]).all(), ("rows differ from the option at 0", what)
    shard_rows = [n] if shard_rows is None else shard_rows
    sp = min((sample_plan(m, k, 1, dim) for m in shard_rows), key=lambda p: p["cap"])
    assert sp["serves"], (what, sp)
    if plain:
        el = np.broadcast_to(np.ones(n, dtype=bool) if eligible is None else eligible, (nq, n))
        for rec in own:
            qi = int(rec["query"])
            assert np.isfinite(rec["D"]), ("a plain query was handed over before its sweep", what, qi, ts)
            within = int((el[qi] & (dists[qi] <= rec["D"] + rec["slack"])).sum())
            assert within + k < sp["cap"], ("a wrong case: the widened radius holds more rows than the first buffers", what,
                                            qi, within, sp)
        assert ts["fallbacks"] == 0 and ts["overflows"] == 0, (what, ts)
        ratio = ts["candidates"] / float(nq * k * sp["stride"])
        RATIO["max"] = max(RATIO["max"], ratio)
        print(what, "candidates / (k stride)", round(ratio, 3), "largest so far", round(RATIO["max"], 3))
        if DEFAULT_TUNABLES:
            masked = bool(filt) or eligible is not None
            assert st["scan_bytes"] == expected_bytes(shard_rows, dim, nq, k, masked), (what, st["scan_bytes"], ts)
    return got, ts, own


# ---- 1. the lattice: rows around a multiple of 16 stride, k beyond the pre-pass, a lone query to several launches ----------

ROWS = (19967, 19968, 19969, 20000)   # 16 * 16 * 78 - 1, + 0, + 1 (a one-row last tile that IS in the sample), about 20 000
LATTICE = [(dim, n, metric) for dim in (64, 768) for n in ROWS for metric in (COS, EUC)]


def lattice_id(c):
    return "d%d-n%d-%s" % (c[0], c[1], MID[c[2]])


@pytest.mark.parametrize("case", LATTICE, ids=[lattice_id(c) for c in LATTICE])
def test_lattice(case):
    dim, n, metric = case
    seed = SEED + dim * 100 + n % 1000
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Qall = orc.synth_vectors(seed + 1, 0, 40, dim) * 0.7
    dall = all_dists(corpus, Qall)
    assert sample_plan(n, 35, 1, dim)["stride"] == 16 and sample_plan(n, 1000, 1, dim)["stride"] == 4
    # (the partial last tile: in the sample of n = 19969 at stride 16 and 4, outside it for the other counts)
    assert (sample_plan(n, 35, 1, dim)["slots"] != sample_plan(n, 35, 1, dim)["sample_rows"]) == (n == 19969)
    with open_tc(dim, metric) as ix:
        ix.synth(n, seed)
        for k in (35, 100, 1000) if dim == 64 else (35, 100):
            for nq in (1, 3, 17, 40):
                what = ("lattice", lattice_id(case), "k", k, "queries", nq)
                checked_call(ix, corpus, Qall[:nq], k, what, dall[:nq])


# ---- 2. masks and tombstones ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", (COS, EUC), ids=["cos", "euc"])
def test_masks_and_tombstones(metric):
    dim, n, nq, k = 64, 20000, 17, 100
    seed = SEED + 5000 + metric
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    dists = all_dists(corpus, Q)
    rng = np.random.default_rng(seed % 1000)
    half = rng.random(n) < 0.5
    with open_tc(dim, metric) as ix:
        ix.synth(n, seed)
        with ix.mask_rows(np.flatnonzero(half)) as mask:   # one resident mask for every query
            got, _, _ = checked_call(ix, corpus, Q, k, ("shared mask", MID[metric]), dists, eligible=half, masks=mask)
        got_w, _, _ = checked_call(ix, corpus, Q, k, ("host words", MID[metric]), dists, eligible=half, allow=np.stack([half] * nq))
        assert tsm.same(got, got_w)
        per = rng.random((nq, n)) < 0.6   # a mask per query
        per[3] = True
        masks = [ix.mask_rows(np.flatnonzero(per[i])) for i in range(nq)]
        try:
            checked_call(ix, corpus, Q, k, ("per-query masks", MID[metric]), dists, eligible=per, masks=masks)
        finally:
            for m in masks:
                m.close()
        dead = np.zeros(n, dtype=bool)
        dead[[0, 5, 16 * 16 + 3, n // 2, n - 1]] = True
        dead[[int(x) for x in got[0][1, :5]]] = True   # rows that were results
        dead[rng.random(n) < 0.1] = True
        ix.tombstone_rows(np.flatnonzero(dead))
        checked_call(ix, corpus, Q, k, ("tombstones", MID[metric]), dists, eligible=~dead)


def test_selective_masks_at_the_rank():
    """The sample of 20 000 rows at stride 16 is the rows of tiles 0, 16, 32, ...  A mask that allows k - 1 of them (and a
    few hundred rows outside the sample) leaves the shard without a key of rank k: handed over; with exactly k: served."""
    dim, n, nq, k, metric = 64, 20000, 3, 35, COS
    seed = SEED + 5100
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    dists = all_dists(corpus, Q)
    in_sample = (np.arange(n) // 16) % 16 == 0
    assert sample_plan(n, k, 1, dim)["stride"] == 16 and int(in_sample.sum()) == sample_plan(n, k, 1, dim)["sample_rows"]
    rng = np.random.default_rng(51)
    others = rng.choice(np.flatnonzero(~in_sample), 300, replace=False)
    picked = rng.choice(np.flatnonzero(in_sample), k, replace=False)
    with open_tc(dim, metric) as ix:
        ix.synth(n, seed)
        for m, served in ((k - 1, False), (k, True)):
            allow = np.zeros(n, dtype=bool)
            allow[others] = True
            allow[picked[:m]] = True
            with ix.mask_rows(np.flatnonzero(allow)) as mask:
                _, ts, own = checked_call(ix, corpus, Q, k, ("rank", m), dists, eligible=allow, plain=served, masks=mask)
            if not served:
                assert ts["fallbacks"] == nq and ts["overflows"] == 0 and ts["queries"] == 0, ts
                assert np.isnan(own["kmax"]).all() and (own["n_entries"] == 0).all()


# ---- 3. rows without a usable sketch, NaN rows, ties, a zero query ------------------------------------------------------------

def planted(seed, n, dim):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dim)).astype(np.float32).astype(np.float64), rng.standard_normal((5, dim))


@pytest.mark.parametrize("metric", (COS, EUC), ids=["cos", "euc"])
def test_exception_rows_inside_the_sample(metric):
    dim, n, k = 64, 8192, 100
    V, Q = planted(61 + metric, n, dim)
    V[16 * 16 + 5] = 0.0          # tile 16 and tile 32: both in the sample at stride 16; beyond the first k rows
    V[32 * 16 + 1, 7] = np.nan
    V[32 * 16 + 2, 0] = np.inf
    corpus = cc.Corpus(orc.encode_rows(V, 32), dim, 32, metric)
    dists = all_dists(corpus, Q)
    with open_tc(dim, metric) as ix:
        ix.load(corpus.packed)
        _, ts, own = checked_call(ix, corpus, Q, k, ("exceptions", MID[metric]), dists)
        exc = set(int(x) for x in ix.sketch_info()["exc_rows"])
        assert {32 * 16 + 1, 32 * 16 + 2} <= exc and ((16 * 16 + 5 in exc) == (metric == COS)), exc


def test_nan_row_among_the_first_k():
    dim, n, k, metric = 64, 8192, 100, COS
    V, Q = planted(63, n, dim)
    V[7, 3] = np.nan
    corpus = cc.Corpus(orc.encode_rows(V, 32), dim, 32, metric)
    dists = all_dists(corpus, Q)
    with open_tc(dim, metric) as ix:
        ix.load(corpus.packed)
        _, ts, own = checked_call(ix, corpus, Q, k, ("nan first",), dists, plain=False)
        assert ts["fallbacks"] == len(Q) and ts["overflows"] == 0, ts
        assert np.isfinite(own["thr"]).all() and (own["certified"] == 0).all()   # (swept, then handed over)
        ix.set_option("tie_mode", 1)
        ix.reset_stats()
        ix.search_topk(Q, k)
        assert ix.sketch_topk_stats()["fallbacks"] == 0


def test_duplicated_rows_tie_at_the_kth_distance():
    dim, n, k, metric = 64, 8192, 35, EUC
    V, Q = planted(64, n, dim)
    Q = Q[:1]
    d0 = ((V - Q[0]) ** 2).sum(axis=1)
    order = np.argsort(d0)
    V[order[-1]] = V[order[k - 1]]   # the k-th nearest row once more, in the farthest row's place
    corpus = cc.Corpus(orc.encode_rows(V, 32), dim, 32, metric)
    dists = all_dists(corpus, Q)
    s = np.sort(dists[0])
    assert s[k - 1] == s[k] and s[k - 2] < s[k - 1] < s[k + 1]
    with open_tc(dim, metric) as ix:
        ix.load(corpus.packed)
        _, ts, own = checked_call(ix, corpus, Q, k, ("tie", "tie_mode 0"), dists, plain=False)
        assert ts["fallbacks"] == 1 and ts["overflows"] == 0 and np.isfinite(own["thr"]).all(), ts
        ix.set_option("tie_mode", 1)   # the fast answer is kept: the same distances, either of the two rows in the last place
        _, ts, _ = checked_call(ix, corpus, Q, k, ("tie", "tie_mode 1"), dists, rows_too=False)
        assert ts["queries"] == 1


def test_zero_cosine_query_and_non_finite_query():
    dim, n, k = 64, 8192, 35
    seed = SEED + 6500
    for metric in (COS, EUC):
        corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
        Q = orc.synth_vectors(seed + 1, 0, 4, dim) * 0.7
        Q[1] = 0.0
        dists = all_dists(corpus, Q)
        with open_tc(dim, metric) as ix:
            ix.synth(n, seed)
            _, ts, own = checked_call(ix, corpus, Q, k, ("zero query", MID[metric]), dists, plain=False)
            want_fb = 1 if metric == COS else 0   # (Euclid: a zero query is ordinary)
            assert ts["fallbacks"] == want_fb and ts["queries"] == 4 - want_fb, ts
            Q2 = Q.copy()
            Q2[2, 5] = np.inf
            ix.reset_stats()
            got = ix.search_topk(Q2, k)
            ts = ix.sketch_topk_stats()
            assert ts["fallbacks"] == want_fb + 1 and ts["queries"] + ts["fallbacks"] == 4, ts
            ix.set_option("sketch_topk_collect", 0)
            got0 = ix.search_topk(Q2, k)
            assert (got[0] == got0[0]).all() and (got[2] == got0[2]).all()


# ---- 4. two shards, float64 rows, the options ---------------------------------------------------------------------------------

def test_two_shards_on_one_device():
    dim, n, nq, k, metric = 64, 20000, 17, 100, COS
    seed = SEED + 7000
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    dists = all_dists(corpus, Q)
    with open_tc(dim, metric, devices=[0, 0]) as ix:
        ix.synth(n, seed)
        per = (n // 2 + 63) // 64 * 64   # (the rows split evenly, in multiples of 64)
        _, ts, own = checked_call(ix, corpus, Q, k, ("two shards",), dists, shard_rows=[per, n - per])
        # tau is the smaller of the shards' bounds, and the shards' samples differ: each shard alone gives another radius
        taus = []
        for lo, hi in ((0, per), (per, n)):
            part = cc.Corpus(corpus.packed[lo:hi], dim, 32, metric)
            with open_tc(dim, metric) as one:
                one.load(part.packed)
                _, _, own1 = checked_call(one, part, Q, k, ("shard alone", lo), dists[:, lo:hi])
                o = np.argsort(own1["query"])   # (less slack: the largest row-to-sketch distance is each handle's own)
                taus.append((own1["thr_min"] - own1["slack"])[o])
        both = (own["thr_min"] - own["slack"])[np.argsort(own["query"])]
        assert (taus[0] != taus[1]).all(), "the shards' bounds differ"
        assert np.allclose(both, np.minimum(taus[0], taus[1]), rtol=1e-12, atol=0), (both, taus)


def test_float64_rows_under_sketch_f64():
    dim, n, nq, k, metric = 64, 8000, 17, 35, COS
    seed = SEED + 7100
    packed = orc.synth_rows(seed, 0, n, dim, 64)
    corpus = cc.Corpus(packed, dim, 64, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    dists = all_dists(corpus, Q)
    ix = ScanIndex(dim, 64, metric, devices=None)
    with ix:
        for name, value in (("sketch_f64", 1), ("sketch", 1), ("sketch_min_rows", 1), ("multi_query", 0),
                            ("sketch_topk_collect", 1)):
            ix.set_option(name, value)
        ix.trace_certificates(True)
        ix.load(packed)
        checked_call(ix, corpus, Q, k, ("float64 rows",), dists)


def test_calls_the_path_does_not_take():
    """k within the pre-pass's lists, a call that shares a sweep, a shard the plan does not serve: nothing is counted."""
    dim, n, metric = 64, 8192, COS
    seed = SEED + 7200
    Q = orc.synth_vectors(seed + 1, 0, 8, dim) * 0.7
    with open_tc(dim, metric) as ix:
        ix.synth(n, seed)
        for k, opts in ((10, {}), (100, {"multi_query": 1}), (1100, {})):   # (8192 rows: 4096 sample rows at stride 2, fewer than 4 k)
            for name, value in opts.items():
                ix.set_option(name, value)
            ix.reset_stats()
            ix.search_topk(Q, k)
            ts = ix.sketch_topk_stats()
            assert ts == dict.fromkeys(ts, 0), (k, opts, ts)
            ix.set_option("multi_query", 0)
        assert not sample_plan(n, 1100, 1, dim)["serves"] and sample_plan(n, 1000, 1, dim)["serves"]
        ix.reset_stats()
        ix.search_topk(Q, 100)
        assert ix.sketch_topk_stats()["queries"] == 8
