"""Groups of queries per row read in the 8-bit one-sweep scan (option "scan_group"): a launch walks its
queries in groups of up to 2 or 4 and reads every row once per group.  The 8-bit row arithmetic is exact integer
arithmetic, so a query's key for a row -- and with it every list, merge, certificate and answer -- is the same however
the queries are grouped: every comparison here is bit for bit (rows, order, float64 distances, NaN == NaN), against
the CPU oracle and against scan_group = 1.  szg_stats.scan_bytes counts one pass per group, which is how a test knows
that the grouped kernel served.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as orc
import scan_lattice as lat
from syzgydb_amd import ScanIndex, SZG_COSINE, SZG_EUCLIDEAN, scan_group_plan

pytestmark = pytest.mark.gpu

SEED = 0x53595A4700002000
DEFAULT_TUNABLES = not os.environ.get("SZG_OPTIONS")   # (an option sweep may change the call plan, never the answers)
CELLS = lat.cells(8)
N_QUERIES = (1, 2, 3, 4, 5, 7, 16, 17, 33)   # partial groups, the 16-query launch boundary, a short call's two parts
KS = (1, 10)
POOL_N = max(N_QUERIES)
ZERO = POOL_N                                 # index of the zero query in the pool
QPL = 16
POOL = ThreadPoolExecutor(8)                  # the oracle's C calls release the interpreter lock
CASES = [(c, m, depth) for c in CELLS for m in (SZG_EUCLIDEAN, SZG_COSINE) for depth in ("small", "deep")]
CASE_IDS = ["%s-%s-%s" % (lat.cell_id(c), "cos" if m == SZG_COSINE else "euc", d) for c, m, d in CASES]


def same(a, b):
    (ra, da, ca), (rb, db, cb) = a, b
    if not (ca == cb).all():
        return False
    for qi in range(len(ca)):
        n = ca[qi]
        x, y = da[qi, :n], db[qi, :n]
        if not (ra[qi, :n] == rb[qi, :n]).all() or not ((x == y) | (np.isnan(x) & np.isnan(y))).all():
            return False
    return True


def assert_oracle(got, want, idx, what):
    r, d, c = got
    for qi, pi in enumerate(idx):
        w_rows, w_dist = want[pi]
        assert [int(x) for x in r[qi, : c[qi]]] == [int(x) for x in w_rows], ("rows differ", what, "query", qi)
        g, w = np.asarray(d[qi, : c[qi]], dtype=np.float64), np.asarray(w_dist, dtype=np.float64)
        assert ((g == w) | (np.isnan(g) & np.isnan(w))).all(), ("distances not bit-equal", what, "query", qi, g, w)


def batch_indices(n, metric):
    """Pool indices of a batch of n queries: the last is the first again (n >= 2), the second is the zero query
    (cosine, n >= 3)."""
    idx = list(range(n))
    if n >= 2:
        idx[n - 1] = 0
    if metric == SZG_COSINE and n >= 3:
        idx[1] = ZERO
    return idx


def effective_group(group, n):
    """A launch of n queries takes no larger a group than it can fill (scan_variant): 1 query -> 1, 2 -> 2."""
    while group > 1 and group // 2 >= n:
        group //= 2
    return group


def call_passes(n, group, qpl=QPL):
    """Passes over the rows of a one-sweep call of n <= 32 queries at the default plan: one batch, from 8 queries on in
    two parts -- all but the last min(4, n / 2) queries, then those (plan_batch) --, each part in launches of qpl
    queries, each launch in groups."""
    assert n <= 32
    parts = [n] if n < 8 else [n - min(4, n // 2), min(4, n // 2)]
    total = 0
    for p in parts:
        for j in range(0, p, qpl):
            m = min(qpl, p - j)
            total += -(-m // effective_group(group, m))
    return total


@functools.lru_cache(maxsize=1)
def corpus(r16, dim, n, seed):
    """The oracle's copy of a cell's rows (shared by the cell's two metrics), synthesised in slices side by side."""
    cuts = np.linspace(0, n, 9).astype(np.int64)
    parts = POOL.map(lambda i: orc.synth_rows(seed, int(cuts[i]), int(cuts[i + 1] - cuts[i]), dim, 8), range(8))
    return np.concatenate(list(parts))


def open_index(dim, bits, metric, group):
    ix = ScanIndex(dim, bits, metric)
    for name, v in (("multi_query", 0), ("sketch", 0), ("query_batch", QPL), ("queries_per_launch", QPL),
                    ("scan_group", group)):
        ix.set_option(name, v)
    return ix


@pytest.mark.parametrize("cell,metric,depth", CASES, ids=CASE_IDS)
def test_grouped_sweep_matches_oracle_and_ungrouped(cell, metric, depth):
    """Every 8-bit cell of the lattice (both row-shape kernels, every any-shape lane map, ragged tails), at the small
    row count (one row step per wave: the general phase) and the deep one (the dense phase over several rows)."""
    dim = cell.dim
    n = cell.small_n if depth == "small" else cell.deep_n
    seed = SEED + cell.r16 * 16 + (7 if depth == "deep" else 0)
    rows = corpus(cell.r16, dim, n, seed)
    pool = np.concatenate([orc.synth_vectors(seed + 1, 0, POOL_N, dim), np.zeros((1, dim))])
    used = range(POOL_N + 1) if metric == SZG_COSINE else range(POOL_N)
    want = {}
    for k in KS:
        jobs = {pi: POOL.submit(orc.search_exact, rows, dim, 8, metric, pool[pi], k=k) for pi in used}
        want[k] = {pi: j.result()[:2] for pi, j in jobs.items()}
    for nq in (4, QPL):   # the cell's images and lists fit LDS at the full group: the plan below holds
        for g in (2, 4):
            assert scan_group_plan(dim, 8, nq, lat.kp_of(10), scan_group=g)["group"] == g
    row_bytes = None
    got, swept = {}, {}
    for group in (1, 2, 4):
        with open_index(dim, 8, metric, group) as ix:
            ix.synth(n, seed)
            assert (ix.read_rows(n - 1, 1) == rows[n - 1:]).all()
            row_bytes = rows.shape[1]
            for k in KS:
                for nq in N_QUERIES:
                    idx = batch_indices(nq, metric)
                    ix.reset_stats()
                    res = ix.search_topk(pool[idx], k)
                    st = ix.stats()
                    what = (lat.cell_id(cell), depth, "scan_group", group, "k", k, "queries", nq)
                    assert_oracle(res, want[k], idx, what)
                    if nq >= 2:   # the query held twice: identical lists, identical answers
                        c = res[2]
                        assert c[0] == c[nq - 1] and (res[0][0, : c[0]] == res[0][nq - 1, : c[0]]).all(), what
                    assert st["mq_queries"] == 0 and st["sketch_queries"] == 0 and st["scan_launches"] > 0, (what, st)
                    got[group, k, nq] = res
                    swept[group, k, nq] = st["scan_bytes"]
    one_pass = n * row_bytes
    for group in (2, 4):
        for k in KS:
            for nq in N_QUERIES:
                what = (lat.cell_id(cell), depth, "scan_group", group, "k", k, "queries", nq)
                assert same(got[group, k, nq], got[1, k, nq]), what
                if nq > 32 or not DEFAULT_TUNABLES:
                    continue
                # scan_group = 1: one pass per query, plus the collect sweeps of queries that escalated -- those keep
                # no lists, are never grouped and are the same whatever the group (the keys are)
                extra = swept[1, k, nq] - nq * one_pass
                assert extra >= 0 and extra % one_pass == 0, what
                assert swept[group, k, nq] == call_passes(nq, group) * one_pass + extra, (what, swept[group, k, nq] / one_pass)


def test_group_steps_aside():
    """scan_group = 4 on a handle whose launches do not qualify: a filter (host words and a resident mask), tombstones,
    k = 80 (lists in LDS) and a radius batch answer as the oracle does, at one pass over the rows per query."""
    cell = [c for c in CELLS if c.shaped == 412][0]
    dim, n, metric = cell.dim, cell.small_n, SZG_EUCLIDEAN
    seed = SEED + 5000
    rows = orc.synth_rows(seed, 0, n, dim, 8)
    Q = orc.synth_vectors(seed + 1, 0, 5, dim)
    nq = Q.shape[0]
    rng = np.random.default_rng(77)
    allow = rng.random(n) < 0.8
    radii = []
    for q in Q:
        alld = orc.all_distances(rows, dim, 8, metric, q)
        radii.append(float(np.quantile(alld[np.isfinite(alld)], 0.05)))
    one_pass = n * rows.shape[1]

    def oracle_topk(k, mask):
        a = None if mask is None else mask.astype(np.uint8)
        return {i: orc.search_exact(rows, dim, 8, metric, Q[i], k=k, allow=a)[:2] for i in range(nq)}

    def passes(ix, run):
        ix.reset_stats()
        res = run()
        st = ix.stats()
        assert st["mq_queries"] == 0 and st["sketch_queries"] == 0, st
        assert st["scan_bytes"] % one_pass == 0
        return res, st["scan_bytes"] // one_pass

    with open_index(dim, 8, metric, 4) as ix:
        ix.synth(n, seed)
        idx = list(range(nq))
        # the grouped kernel does serve this handle: 5 unmasked queries at k = 10 are two passes
        res, p = passes(ix, lambda: ix.search_topk(Q, 10))
        assert_oracle(res, oracle_topk(10, None), idx, "unmasked k = 10")
        if DEFAULT_TUNABLES:
            assert p == 2, p
        # lists in LDS
        res, p = passes(ix, lambda: ix.search_topk(Q, 80))
        assert_oracle(res, oracle_topk(80, None), idx, "k = 80")
        assert p >= nq
        ix.set_option("scan_group", 1)
        assert passes(ix, lambda: ix.search_topk(Q, 80))[1] == p
        ix.set_option("scan_group", 4)
        # a filter, from the host and resident
        want = oracle_topk(10, allow)
        res, p = passes(ix, lambda: ix.search_topk(Q, 10, allow=np.tile(allow, (nq, 1))))
        assert_oracle(res, want, idx, "allow=")
        assert p >= nq
        with ix.mask(allow) as m:
            res, pm = passes(ix, lambda: ix.search_topk(Q, 10, masks=m))
            assert_oracle(res, want, idx, "masks=")
            assert pm == p
            ix.set_option("scan_group", 1)
            assert passes(ix, lambda: ix.search_topk(Q, 10, masks=m))[1] == p
            ix.set_option("scan_group", 4)
        # a radius batch (collect sweeps)
        hits, p = passes(ix, lambda: ix.search_radius_batch(Q, radii))
        for qi in range(nq):
            w_rows, w_dist = orc.search_exact(rows, dim, 8, metric, Q[qi], radius=radii[qi])[:2]
            assert [int(x) for x in hits[qi][0]] == [int(x) for x in w_rows], ("radius", qi)
            assert (np.asarray(hits[qi][1]) == np.asarray(w_dist)).all(), ("radius", qi)
        assert p >= nq
        ix.set_option("scan_group", 1)
        assert passes(ix, lambda: ix.search_radius_batch(Q, radii))[1] == p
        ix.set_option("scan_group", 4)
        # tombstones
        live = np.ones(n, dtype=bool)
        for r in (0, 5, n // 2, n - 1):
            ix.tombstone(int(r))
            live[r] = False
        res, p = passes(ix, lambda: ix.search_topk(Q, 10))
        assert_oracle(res, oracle_topk(10, live), idx, "tombstones")
        assert p >= nq
        ix.set_option("scan_group", 1)
        assert passes(ix, lambda: ix.search_topk(Q, 10))[1] == p


# ---- the sketch pre-pass (float32 rows behind an 8-bit sketch) ------------------------------------------------------------

SK_ROWS = 70000


@functools.lru_cache(maxsize=1)
def float_corpus(dim):
    rng = np.random.default_rng(2100 + dim)
    V = rng.standard_normal((SK_ROWS, dim)).astype(np.float32).astype(np.float64)
    return orc.encode_rows(V, 32), rng.standard_normal((40, dim))


def search_modes(ix, Q, k, modes):
    out = {}
    for name, opts in modes:
        for o, v in opts.items():
            ix.set_option(o, v)
        ix.reset_stats()
        res = ix.search_topk(Q, k)
        st = ix.stats()
        out[name] = (res, st["sketch_queries"], st["sketch_fallbacks"], st["mq_queries"])
    return out


SK_MODES = (("g1", {"sketch": 1, "scan_group": 1}), ("g2", {"sketch": 1, "scan_group": 2}),
            ("g4", {"sketch": 1, "scan_group": 4}), ("off", {"sketch": 0, "scan_group": 1}))


@pytest.mark.parametrize("metric", [SZG_COSINE, SZG_EUCLIDEAN], ids=["cos", "euc"])
@pytest.mark.parametrize("dim", [768, 100])
def test_sketch_prepass_grouped(dim, metric):
    """The sketch sweep (8-bit rows of the float32 collection) in groups: the answers of scan_group = 1 and of the full
    sweep, every query counted by the pre-pass, the same queries handed over whatever the group."""
    rows, Qall = float_corpus(dim)
    with ScanIndex(dim, 32, metric) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        for nq in (1, 5, 16, 40):
            res = search_modes(ix, Qall[:nq], 10, SK_MODES)
            for name in ("g2", "g4", "off"):
                assert same(res[name][0], res["g1"][0]), (name, nq)
            for name in ("g1", "g2", "g4"):
                assert res[name][1] + res[name][2] == nq and res[name][3] == 0, (name, nq, res[name][1:])
                assert res[name][1:3] == res["g1"][1:3], (name, nq)


def test_sketch_short_lists_fall_back_alike():
    """sketch_list = 8 and one block that holds 40 of the query's best rows, more than its list keeps: the drop bound
    binds and the query is handed to the full sweep -- identically for every group size."""
    dim, n, n_close = 48, 65536, 40
    rng = np.random.default_rng(2200)
    V = rng.standard_normal((n, dim))
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)
    for i in range(n_close):   # rows [0, 40): all in the sweep's first block, at distinct angular distances from q
        u = rng.standard_normal(dim)
        u -= u.dot(q) * q
        u /= np.linalg.norm(u)
        a = np.pi * (0.02 + 0.001 * i)
        V[i] = np.cos(a) * q + np.sin(a) * u
    rows = orc.encode_rows(V, 32)
    Q = np.stack([q, q * 2.0, q + 1e-4 * np.arange(dim) / dim, rng.standard_normal(dim), q * 0.5])
    k = 10
    with ScanIndex(dim, 32, SZG_COSINE) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        ix.set_option("sketch_list", 8)
        res = search_modes(ix, Q, k, SK_MODES)
        for qi in range(Q.shape[0]):
            o_rows, o_dist, _ = orc.search_exact(rows, dim, 32, SZG_COSINE, Q[qi], k=k)
            r, d, c = res["g1"][0]
            assert [int(x) for x in r[qi, : c[qi]]] == [int(x) for x in o_rows], qi
            assert (d[qi, : c[qi]] == o_dist).all(), qi
        assert res["g1"][2] >= 4, res["g1"][1:]          # the four queries next to the crowded block are handed over
        for name in ("g2", "g4", "off"):
            assert same(res[name][0], res["g1"][0]), name
        for name in ("g2", "g4"):
            assert res[name][1:3] == res["g1"][1:3], (name, res[name][1:], res["g1"][1:])


def test_option_range():
    with ScanIndex(16, 8, SZG_COSINE) as ix:
        for v in (0, 1, 2, 4):
            ix.set_option("scan_group", v)
        for v in (-1, 3, 5, 8):
            with pytest.raises(Exception):
                ix.set_option("scan_group", v)
