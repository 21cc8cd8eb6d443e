"""The matrix sketch sweep (kernels_scan_mx.hip; option sketch_matrix): float32 handles behind their 8-bit sketch, whose
one-sweep launches score up to 16 queries per row read on the matrix cores.

Per case: the certificate chain on the trace (K_s, L_s with the drop bound, D, S -- cert_check) and the answers against the
oracle; the same answers under sketch_matrix = 1 (the grouped VALU kernels) and sketch = 0; and the pass count of
szg_stats.scan_bytes, which is how a test knows the matrix kernel ran: one pass per launch of up to 16 queries, where the
grouped kernels make one per 4.

How a call splits into launches (scan_topk.cpp, plan_batch and enqueue_topk; default tunables): up to 32 queries are ONE
batch, from 8 queries on in two parts -- all but the last min(4, n / 2), then those; longer calls go in batches of 16 with
a first and a last batch of 4.  Every launch holds at most 16 queries.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import ScanIndex, _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import scan_plan, scan_matrix_plan, scan_share_plan

pytestmark = pytest.mark.gpu

SEED = 0x53595A470000B000
EUC, COS = 0, 1
MID = {EUC: "euc", COS: "cos"}
POOL = ThreadPoolExecutor(8)   # the oracle's C calls release the interpreter lock
DEFAULT_TUNABLES = not os.environ.get("SZG_OPTIONS")   # (an option sweep may change the call plan, never the answers)
MARGINS = cc.Margins()
TOTALS = {d: [0, 0] for d in (64, 192, 384, 768)}   # dim -> [keys checked, queries settled] over this file's calls


def sketch_kp(k):
    """Candidates per query of a sketch sweep (SketchCall::run: kk = k + sketch_extra = k + 30; kk + max(16, kk / 2))."""
    kk = k + 30
    return kk + max(16, kk // 2)


def launch_sizes(nq):
    """Queries per launch of a one-sweep call of nq queries under default tunables (see the module's docstring)."""
    if nq <= 32:
        parts = [nq] if nq < 8 else [nq - min(4, nq // 2), min(4, nq // 2)]
    else:
        parts, q0 = [], 0
        while q0 < nq:
            left = nq - q0
            n = min(16, left)
            if left > 4:
                n = min(n, 4) if q0 == 0 else (left - 4 if left <= 20 else n)
            parts.append(n)
            q0 += n
    out = []
    for p in parts:
        out += [16] * (p // 16) + ([p % 16] if p % 16 else [])
    return out


def matrix_passes(nq):
    return sum(-(-n // 16) for n in launch_sizes(nq))   # ceil(n / 16) per launch: one each


def grouped_passes(nq):
    return sum(-(-n // 4) for n in launch_sizes(nq))


def test_launch_plan_of_this_file():
    assert launch_sizes(3) == [3] and launch_sizes(16) == [12, 4] and launch_sizes(17) == [13, 4]
    assert launch_sizes(40) == [4, 16, 16, 4]
    for nq in (3, 16, 17, 40):   # every launch of the lattice's calls is one the matrix sweep takes under automatic
        assert min(launch_sizes(nq)) >= 3
    assert [matrix_passes(q) for q in (3, 16, 17, 40)] == [1, 2, 2, 4]
    assert [grouped_passes(q) for q in (3, 16, 17, 40)] == [1, 4, 5, 10]


def test_call_plan_hook_counts_the_launches_the_card_makes():
    """The call-plan hook (szg_debug_scan_share) and the launch path compute from the same plan (sketch_plan.h): for calls
    of 7, 8, 17, 32 and 40 queries over 20 000 rows of 64 dimensions (cosine, k = 10, lists of 8) the launches the
    statistics count and the passes of scan_bytes are the hook's and this file's launch_sizes -- [7], [4, 4], [13, 4],
    [16, 12, 4] and [4, 16, 16, 4], the two parts of a short call included.  Exact where the sketch settled every query
    (assert_pass_count's guard: a query handed over adds sweeps of the float32 rows)."""
    dim, k, n = 64, 10, 20000
    rng = np.random.default_rng(5200)
    V = rng.standard_normal((n, dim)).astype(np.float32).astype(np.float64)
    Qall = rng.standard_normal((40, dim))
    assert [launch_sizes(q) for q in (7, 8, 32)] == [[7], [4, 4], [16, 12, 4]]
    with open_sketched(dim, COS, devices=[0], sketch_list=8) as ix:
        ix.load(orc.encode_rows(V, 32))
        ix.trace_certificates(False)
        for nq in (7, 8, 17, 32, 40):
            what = ("call plan", nq)
            hook = scan_share_plan(dim, 8, nq, kp=8)
            assert hook["launches"] == len(launch_sizes(nq)) and hook["passes"] == matrix_passes(nq), (what, hook)
            ix.reset_stats()
            ix.search_topk(Qall[:nq], k)
            st = ix.stats()
            print(what, "launches", st["scan_launches"], "passes", sketch_passes(st, n, dim, what), "hook", hook["launches"],
                  hook["passes"], "settled", st["sketch_queries"], "of", nq)
            assert_pass_count(st, n, dim, nq, hook["passes"], what)
            if DEFAULT_TUNABLES and st["sketch_queries"] == nq and st["escalations"] == 0 and st["full_replays"] == 0:
                assert st["scan_launches"] == hook["launches"] == len(launch_sizes(nq)), (what, st, hook)
                assert sketch_passes(st, n, dim, what) == hook["passes"] == matrix_passes(nq), (what, st, hook)


def rows_per_step(dim):
    p = scan_plan(dim, 8, 1 << 22, kp=sketch_kp(10))
    assert p["tiled"]
    return p["grid"] * (p["block"] // 64) * 16


def n_rows_of(dim, spec):
    return spec if isinstance(spec, int) else int(spec[1:]) * rows_per_step(dim) + 77


@functools.lru_cache(maxsize=2)
def synth_corpus(seed, n, dim):
    cuts = np.linspace(0, n, 9).astype(np.int64)
    parts = POOL.map(lambda i: orc.synth_rows(seed, int(cuts[i]), int(cuts[i + 1] - cuts[i]), dim, 32), range(8))
    return np.concatenate(list(parts))


def open_sketched(dim, metric, devices=None, **options):
    ix = ScanIndex(dim, 32, metric, devices=devices)
    for name, value in dict({"sketch": 1, "sketch_min_rows": 1, "multi_query": 0, "scan_group": 0, "sketch_matrix": 0},
                            **options).items():
        ix.set_option(name, value)
    ix.trace_certificates(True)
    return ix


def same(a, b):
    return all((x == y).all() for x, y in zip(a, b))


def assert_answers(got, packed, dim, metric, Q, k, eligible, what):
    r, d, cnt = got
    allow = None if eligible is None else eligible.astype(np.uint8)
    want = POOL.map(lambda q: orc.search_exact(packed, dim, 32, metric, q, k=k, allow=allow)[:2], Q)
    for qi, (w_rows, w_dist) in enumerate(want):
        assert [int(x) for x in r[qi, : cnt[qi]]] == [int(x) for x in w_rows], ("rows differ", what, qi)
        g = d[qi, : cnt[qi]]
        assert ((g == w_dist) | (np.isnan(g) & np.isnan(w_dist))).all(), ("distances not bit-equal", what, qi)


def certified_call(ix, corpus, Q, k, what, dists=None, eligible=None, **filt):
    """One top-k call through the sketch: K_s (every list key within key_eps of its float64 key), L_s (every eligible
    sketched row outside the lists at or above lb, the drop bound included), D and S on its sketch records, K, L, C on the
    records of the queries it handed over, and the answers against the oracle.
    -> (answers, stats, keys checked, queries settled, dists)"""
    Q = np.atleast_2d(Q)
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
    s = cc.check(corpus, Q, recs, ents, dropped, eligible=eligible, dists=dists, margins=MARGINS, what=what,
                 sketch=(sk_corpus, info["gscale"], info["exc_rows"]))
    assert s.skipped == 0, ("candidates without a bound on a corpus that plants no bad row", what, sorted(s.skipped_rows)[:8])
    # (a list that holds every row leaves no row out: lb is +inf and there is no bound to check the keys against)
    assert s.checked > 0 or not np.isfinite(sk["thr_min"]).any(), ("no key was checked", what)
    assert_answers(got, corpus.packed, corpus.dim, corpus.metric, Q, k, eligible, what)
    TOTALS[corpus.dim][0] += s.checked
    TOTALS[corpus.dim][1] += int((sk["certified"] == 1).sum())
    return got, st, s.checked, int((sk["certified"] == 1).sum()), dists


def sketch_passes(st, n, dim, what):
    """Passes over the rows, in sketch rows (dim bytes each): a sweep of the float32 rows of a query handed over counts 4."""
    assert st["scan_bytes"] % (n * dim) == 0, (what, st)
    return st["scan_bytes"] // (n * dim)


def assert_pass_count(st, n, dim, nq, want, what):
    """The sketch sweeps made `want` passes.  Sweeps of the float32 rows (queries handed over) add multiples of 4, so
    the count holds modulo 4 always and exactly when the sketch settled every query."""
    if not DEFAULT_TUNABLES:
        return
    p = sketch_passes(st, n, dim, what)
    print(what, "passes (sketch rows)", p, "expected of the sketch sweeps", want, "settled", st["sketch_queries"], "of", nq)
    assert p % 4 == want % 4 and p >= want, (what, p, want)
    if st["sketch_queries"] == nq and st["escalations"] == 0 and st["full_replays"] == 0:
        assert p == want, (what, p, want)


# (dim, rows: a count or "s<whole steps of the launch>" plus 77, queries, k, metric) -- every value of every axis, each
# kernel form (64, 192: any-steps; 384, 768: shaped) at a row count below, at and above one tile and over several steps
CASES = [
    (64, 15, 3, 10, COS), (64, 16, 17, 1, EUC), (64, 17, 40, 10, EUC), (64, "s1", 16, 10, COS), (64, "s3", 3, 1, EUC),
    (192, 15, 16, 1, EUC), (192, 17, 3, 10, COS), (192, "s1", 40, 10, EUC), (192, "s3", 17, 10, COS),
    (384, 16, 40, 10, COS), (384, 15, 16, 10, EUC), (384, "s1", 17, 1, COS), (384, "s3", 40, 10, EUC),
    (768, 15, 17, 10, EUC), (768, 17, 3, 1, COS), (768, 16, 40, 10, COS), (768, "s1", 16, 10, COS), (768, "s3", 17, 10, EUC),
]


def case_id(c):
    dim, rows, nq, k, metric = c
    return "d%d-n%s-q%d-k%d-%s" % (dim, rows, nq, k, MID[metric])


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_certificates_answers_passes(case):
    dim, rows, nq, k, metric = case
    n = n_rows_of(dim, rows)
    seed = SEED + dim * 100 + (n % 1000) + k
    corpus = cc.Corpus(synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    what = ("matrix", case_id(case), "rows", n)
    for n_l in launch_sizes(nq):   # the plan: every launch of this call is the matrix sweep's
        assert scan_matrix_plan(dim, 8, n_l, kp=8)["serves"]
    # one tile or two: the lists of kp entries hold every row (no bound to check); at k = 1 lists of 8 leave rows out
    lst = 8 if isinstance(rows, int) and k == 1 else 0
    with open_sketched(dim, metric, sketch_list=lst) as ix:
        ix.synth(n, seed)
        assert (ix.read_rows(n - 1, 1) == corpus.packed[n - 1:]).all()   # device synthesis == the oracle's
        got, st, checked, settled, dists = certified_call(ix, corpus, Q, k, what)
        assert st["sketch_queries"] + st["sketch_fallbacks"] == nq and st["mq_queries"] == 0, (what, st)
        assert_pass_count(st, n, dim, nq, matrix_passes(nq), what)
        ix.set_option("sketch_matrix", 1)
        got1, st1, _, settled1, _ = certified_call(ix, corpus, Q, k, what + ("sketch_matrix = 1",), dists=dists)
        assert same(got, got1), ("answers differ from the grouped kernels'", what)
        assert_pass_count(st1, n, dim, nq, grouped_passes(nq), what + ("sketch_matrix = 1",))
        ix.set_option("sketch", 0)
        ix.reset_stats()
        got0 = ix.search_topk(Q, k)
        assert same(got, got0), ("answers differ from sketch = 0", what)
        print(what, "keys checked", checked, "settled", settled, "grouped", settled1)


@pytest.mark.parametrize("dim", (768, 384))
@pytest.mark.parametrize("metric", (COS, EUC), ids=["cos", "euc"])
def test_gaussian_rows_settle(dim, metric):
    """6 007 gaussian rows: the sketch settles as many queries as under sketch_matrix = 1 -- under cosine 16 of 16 and
    17 of 17, at exactly one pass per launch."""
    n, k = 6007, 10
    rng = np.random.default_rng(3100 + dim)
    V = rng.standard_normal((n, dim)).astype(np.float32).astype(np.float64)
    Qall = rng.standard_normal((17, dim))
    corpus = cc.Corpus(orc.encode_rows(V, 32), dim, 32, metric)
    with open_sketched(dim, metric) as ix:
        ix.load(corpus.packed)
        for nq in (16, 17):
            what = ("gaussian", dim, MID[metric], nq)
            res = {}
            for sm in (1, 0):
                ix.set_option("sketch_matrix", sm)
                got, st, checked, settled, _ = certified_call(ix, corpus, Qall[:nq], k, what + ("sketch_matrix", sm))
                res[sm] = (got, st["sketch_queries"])
                assert_pass_count(st, n, dim, nq, matrix_passes(nq) if sm == 0 else grouped_passes(nq), what + (sm,))
            assert same(res[0][0], res[1][0]), what
            assert res[0][1] == res[1][1], ("the sketch settles other counts under the two kernels", what, res[0][1], res[1][1])
            if metric == COS:   # (Euclidean: the grouped kernels settle 15 of 16 of these queries at 768 dimensions)
                assert res[0][1] == nq, (what, res[0][1])
                if DEFAULT_TUNABLES:   # every query settled: the count is exact
                    assert sketch_passes(st, n, dim, what) == matrix_passes(nq)


def test_fallbacks_keep_their_kernels():
    """A filter, a tombstone, k = 34 (kp = 96 candidates per query) and scan_group = 4: the matrix sweep steps aside --
    identical answers and the pass counts of sketch_matrix = 1, read in the same test."""
    dim, metric, k, nq = 384, COS, 10, 16
    n = rows_per_step(dim) + 77
    seed = SEED + 9000
    corpus = cc.Corpus(synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    allow = np.arange(n) % 5 != 2

    def run(ix, kk, eligible=None, **filt):
        ix.reset_stats()
        got = ix.search_topk(Q, kk, **filt)
        st = ix.stats()
        assert_answers(got, corpus.packed, dim, metric, Q, kk, eligible, ("fall-back", kk, sorted(filt)))
        return got, (st["scan_launches"], st["scan_bytes"], st["sketch_queries"], st["sketch_fallbacks"])

    with open_sketched(dim, metric) as ix:
        ix.synth(n, seed)
        seen = {}
        for sm in (1, 0):
            ix.set_option("sketch_matrix", sm)
            seen[sm, "k34"] = run(ix, 34)
            seen[sm, "filter"] = run(ix, k, eligible=allow, allow=np.stack([allow] * nq))
            ix.set_option("scan_group", 4)
            seen[sm, "g4"] = run(ix, k)
            ix.set_option("scan_group", 0)
            seen[sm, "plain"] = run(ix, k)
        for leg in ("k34", "filter", "g4"):
            assert same(seen[0, leg][0], seen[1, leg][0]), leg
            assert seen[0, leg][1] == seen[1, leg][1], ("pass counts moved on a launch the matrix sweep does not serve", leg, seen[0, leg][1], seen[1, leg][1])
        assert same(seen[0, "plain"][0], seen[1, "plain"][0])
        if DEFAULT_TUNABLES:   # (the floor: on this handle the option does change the unmasked k = 10 call)
            assert seen[0, "plain"][1][1] < seen[1, "plain"][1][1], seen
        dead = np.zeros(n, dtype=bool)
        dead[[0, 5, n // 2, n - 1]] = True
        ix.tombstone_rows(np.flatnonzero(dead))
        for sm in (1, 0):
            ix.set_option("sketch_matrix", sm)
            seen[sm, "dead"] = run(ix, k, eligible=~dead)
        assert same(seen[0, "dead"][0], seen[1, "dead"][0])
        assert seen[0, "dead"][1] == seen[1, "dead"][1], (seen[0, "dead"][1], seen[1, "dead"][1])


def crowded_block(seed, n, dim, n_close=40):
    """Random rows, except rows [0, n_close) -- all in the sweep's first block (16 rows per wave, 4 waves) -- at distinct
    angular distances 0.02, 0.021, ... from the query q"""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, dim))
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)
    for i in range(n_close):
        u = rng.standard_normal(dim)
        u -= u.dot(q) * q
        u /= np.linalg.norm(u)
        a = np.pi * (0.02 + 0.001 * i)
        V[i] = np.cos(a) * q + np.sin(a) * u
    return V, q


def test_drop_bound_crowded_block():
    """40 of a query's best rows inside one block's rows, sketch_list = 8: the query is handed over or settles -- either
    way L_s holds against the recorded lb (cert_check) and the answer is the oracle's."""
    dim, k, n = 64, 10, 20000
    V, q = crowded_block(1400, n, dim)
    corpus = cc.Corpus(orc.encode_rows(V, 32), dim, 32, COS)
    Q = np.stack([q, q * 2.0, q + 1e-4 * np.arange(dim) / dim])
    with open_sketched(dim, COS, sketch_list=8) as ix:
        ix.load(corpus.packed)
        got, st, checked, settled, dists = certified_call(ix, corpus, Q, k, ("drop bound", "matrix"))
        assert st["sketch_queries"] + st["sketch_fallbacks"] == 3, st
        assert_pass_count(st, n, dim, 3, 1, ("drop bound",))
        ix.set_option("sketch_matrix", 1)
        got1, st1, _, settled1, _ = certified_call(ix, corpus, Q, k, ("drop bound", "grouped"), dists=dists)
        assert same(got, got1)
        print("drop bound: settled", settled, "grouped", settled1)


def test_last_tile_rows_never_appear():
    """17 rows in a handle that held 32 whose rows 17 .. 31 would win every query: the tile's bytes past n_rows stay as
    allocated, are read and must be discarded."""
    dim, k, nq = 64, 10, 3
    rng = np.random.default_rng(4100)
    Q = rng.standard_normal((nq, dim))
    for metric in (COS, EUC):
        V = rng.standard_normal((32, dim))
        V[17:] = Q.mean(axis=0) * (1.0 + 0.01 * np.arange(15))[:, None]   # closest to every query, by far
        packed = orc.encode_rows(V, 32)
        with open_sketched(dim, metric) as ix:
            ix.load(packed)
            r32, _, _ = ix.search_topk(Q, k)
            assert (r32[:, 0] >= 17).all(), ("the planted rows do not win", metric, r32[:, 0])
        with open_sketched(dim, metric) as ix:
            ix.load(packed)
            ix.search_topk(Q, k)   # (the sketch of the 32 rows is built)
            ix.certificates()      # (that call's records: read and dropped)
            ix.load(packed[:17])
            corpus = cc.Corpus(packed[:17], dim, 32, metric)
            got, st, checked, settled, _ = certified_call(ix, corpus, Q, k, ("last tile", MID[metric]))
            assert (got[0][:, :k] < 17).all(), (metric, got[0])
            assert_pass_count(st, 17, dim, nq, 1, ("last tile", MID[metric]))


def test_margins():
    """What the tests above measured: every K_s ratio |key - real| / (ub - key) is at most 1; per dimension (kernel
    form) keys were checked and queries settled."""
    for dim, (checked, settled) in TOTALS.items():
        assert checked > 0 and settled > 0, (dim, checked, settled)
    for what, ratio in MARGINS.worst.items():
        assert ratio <= 1.0, (what, ratio)
    for line in MARGINS.lines():
        print(line)
