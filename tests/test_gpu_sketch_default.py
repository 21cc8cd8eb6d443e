"""The sketch pre-pass as the default ("sketch" option 2, automatic): float32 handles of >= 65 536 rows answer
one-query-per-sweep searches through the 8-bit sketch, step aside where it does not pay or does not fit, and
answer exactly what the reference loop answers either way."""
import os

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import ScanIndex, SZG_COSINE, SZG_EUCLIDEAN
from syzgydb_amd.index import sample_plan

pytestmark = pytest.mark.gpu
DEFAULT_TUNABLES = not os.environ.get("SZG_OPTIONS")
N = 65536


def check(ix, rows, dim, Q, k, metric=SZG_COSINE, allow=None, live=None):
    kw = {}
    if allow is not None:
        kw["allow"] = np.tile(allow, (Q.shape[0], 1))
    r, d, c = ix.search_topk(Q, k, **kw)
    m = None
    if allow is not None or live is not None:
        m = np.ones(rows.shape[0], bool)
        if allow is not None:
            m &= allow
        if live is not None:
            m &= live
        m = m.astype(np.uint8)
    for qi in range(Q.shape[0]):
        o_rows, o_dist, _ = orc.search_exact(rows, dim, 32, metric, Q[qi], k=k, allow=m)
        assert c[qi] == len(o_rows), qi
        assert [int(x) for x in r[qi, : c[qi]]] == [int(x) for x in o_rows], qi
        got, want = d[qi, : c[qi]], o_dist
        assert ((got == want) | (np.isnan(got) & np.isnan(want))).all(), qi


def through_sketch(ix):
    st = ix.stats()
    return st["sketch_queries"] + st["sketch_fallbacks"]


@pytest.mark.parametrize("metric", [SZG_COSINE, SZG_EUCLIDEAN])
@pytest.mark.parametrize("k", [1, 10, 34])
def test_default_takes_the_sketch(metric, k):
    dim = 48
    rng = np.random.default_rng(900 + k + 7 * metric)
    V = rng.standard_normal((N, dim))
    rows = orc.encode_rows(V, 32)
    Q = rng.standard_normal((6, dim))
    with ScanIndex(dim, 32, metric) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        check(ix, rows, dim, Q, k, metric)                  # one call, one sweep per query
        for qi in range(2):                                 # lone calls
            check(ix, rows, dim, Q[qi : qi + 1], k, metric)
        if DEFAULT_TUNABLES:
            st = ix.stats()
            assert st["sketch_queries"] + st["sketch_fallbacks"] == 8
            assert st["sketch_queries"] >= 6


def test_off_and_forced_on():
    dim = 32
    rows = orc.synth_rows(910, 0, N, dim, 32)
    Q = orc.synth_vectors(911, 0, 4, dim)
    with ScanIndex(dim, 32, SZG_COSINE) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        ix.set_option("sketch", 0)
        check(ix, rows, dim, Q, 10)
        assert through_sketch(ix) == 0
        ix.set_option("sketch", 1)
        check(ix, rows, dim, Q, 10)
        assert through_sketch(ix) == 4
    with pytest.raises(Exception):
        with ScanIndex(dim, 32, SZG_COSINE) as ix:
            ix.set_option("sketch", 3)


def clustered(seed, n, dim):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((40, dim))
    V = centers[rng.integers(0, 40, n)] + rng.standard_normal((n, dim)) * 1e-3
    Q = centers[rng.integers(0, 40, 80)] + rng.standard_normal((80, dim)) * 1e-3
    return V, Q


def test_auto_steps_aside_on_tight_clusters_and_comes_back():
    """Rows within 1e-3 of each other in angle: the bound cannot separate them.  Forced on, every query still goes
    through the sketch; in auto mode the handle stops after a window of hand-overs, and a mutation re-arms it."""
    dim = 96
    V, Q = clustered(32, N, dim)
    rows = orc.encode_rows(V, 32)
    with ScanIndex(dim, 32, SZG_COSINE) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        ix.set_option("sketch", 1)
        check(ix, rows, dim, Q[:10], 10)
        assert through_sketch(ix) == 10                    # forced on: never steps aside
        ix.set_option("sketch", 2)
        ix.reset_stats()
        for qi in range(Q.shape[0]):                       # 80 lone calls
            check(ix, rows, dim, Q[qi : qi + 1], 10)
        st = ix.stats()
        if DEFAULT_TUNABLES:
            assert st["sketch_fallbacks"] >= 16
            assert 64 <= through_sketch(ix) < 80           # stepped aside after a full window
            before = through_sketch(ix)
            check(ix, rows, dim, Q[:4], 10)
            assert through_sketch(ix) == before            # still aside
            ix.tombstone(3)                                # a mutation re-arms it
            live = np.ones(N, bool)
            live[3] = False
            check(ix, rows, dim, Q[:4], 10, live=live)
            assert through_sketch(ix) == before + 4


def test_mutations_masks_odd_rows_and_two_shards():
    dim = 64
    rng = np.random.default_rng(920)
    n = N + 4096
    V = rng.standard_normal((n + 3000, dim))
    V[2005] = 0.0                                          # (beyond the first k rows: a NaN there sends every
    V[2006, 3] = np.inf                                    # query to the full sweep, test_gpu_sketch.py has that)
    V[2007, 9] = np.nan
    V[50] = V[51]
    rows = orc.encode_rows(V, 32)
    Q = rng.standard_normal((10, dim))
    Q[3] = V[50] + rng.standard_normal(dim) * 1e-6
    allow = rng.random(n + 3000) < 0.5
    for devices in (None, [0, 0]):
        kw = {} if devices is None else {"devices": devices}
        with ScanIndex(dim, 32, SZG_COSINE, **kw) as ix:
            R = rows.copy()
            ix.load(R[:n])
            ix.set_option("multi_query", 0)
            check(ix, R[:n], dim, Q, 10)
            check(ix, R[:n], dim, Q, 10, allow=allow[:n])
            ix.append(R[n:])
            check(ix, R, dim, Q, 10)
            for r0 in (10, n - 5, n + 2500):
                v = Q[1] * 3.0 + rng.standard_normal(dim) * 0.01
                R[r0] = orc.encode_rows(v.reshape(1, -1), 32)[0]
                ix.overwrite(r0, R[r0])
            check(ix, R, dim, Q, 10)
            live = np.ones(n + 3000, bool)
            for r0 in (10, 4000, 77, n + 1):
                ix.tombstone(r0)
                live[r0] = False
            check(ix, R, dim, Q, 10, live=live)
            check(ix, R, dim, Q, 10, allow=allow, live=live)
            if DEFAULT_TUNABLES:
                assert ix.stats()["sketch_queries"] > 0


def test_refused_allocation_leaves_the_handle_working():
    dim = 32
    rows = orc.synth_rows(930, 0, N, dim, 32)
    Q = orc.synth_vectors(931, 0, 4, dim)
    with ScanIndex(dim, 32, SZG_COSINE) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        ix.set_option("force_sketch_nomem", 1)
        check(ix, rows, dim, Q, 10)                        # no error: the full sweep answers
        assert through_sketch(ix) == 0
        ix.set_option("force_sketch_nomem", 0)
        check(ix, rows, dim, Q, 10)
        assert through_sketch(ix) == 0                     # aside until the next load
        ix.load(rows)
        check(ix, rows, dim, Q, 10)
        if DEFAULT_TUNABLES:
            assert through_sketch(ix) == 4


def served_beyond_the_prepass(ix):
    """Queries that radius searches and top-k searches of large k took through the sketch: settled and handed over."""
    st, ts = ix.stats(), ix.sketch_topk_stats()
    return st["sketch_radius_queries"] + st["sketch_radius_fallbacks"], ts["queries"] + ts["fallbacks"]


@pytest.mark.parametrize("dim", [32, 64])
@pytest.mark.parametrize("metric", [SZG_COSINE, SZG_EUCLIDEAN], ids=["cos", "euc"])
def test_refused_allocation_on_the_radius_and_large_k_paths(metric, dim):
    """The hook of the test above through the other two entry points of the sketch: a radius call, and a top-k call whose
    k is beyond the pre-pass's lists (sketch_topk_collect).  2 005 rows (no multiple of 16) in two shards on one device, 5
    queries, one of them masked: under sketch = 1 all three entry points report the refusal; once the hook is cleared
    and the rows are loaded again the paths serve.  Two things the shape alone does not reach.  Auto mode keeps no
    sketch below 65 536 rows -- at 2 005 it steps aside whatever the hook says -- so the auto-mode half runs at 65 536
    rows as well, the smallest count at which the refusal is met inside the entry frame: no error, the oracle's answers,
    nothing counted as served.  And the sample pass of the large-k path takes sketch rows of whole 64-byte steps only:
    at dim 32 the entry frame's "does not serve" clause sends such a call the way it goes without the option -- its
    counters stay 0 by that rule, which is asserted from the sample plan -- and dim 64 is where they rise."""
    nq, k_big = 5, 100

    def expected(n):   # (radius queries, large-k queries) through the sketch once it serves
        per = (n // 2 + 63) // 64 * 64
        plans = [sample_plan(rows, k_big, 1, dim)["serves"] for rows in (per, n - per)]
        assert all(plans) == (dim == 64) and any(plans) == (dim == 64), plans
        return nq, nq if all(plans) else 0

    def case(n, seed):
        rows = orc.synth_rows(seed, 0, n, dim, 32)
        Q = orc.synth_vectors(seed + 1, 0, nq, dim)
        allow = np.ones((nq, n), bool)
        allow[2] = np.random.default_rng(seed).random(n) < 0.5
        radii = np.zeros(nq)
        want_r, want_k = [], []
        for qi in range(nq):
            m = allow[qi].astype(np.uint8)
            d = np.sort(orc.all_distances(rows, dim, 32, metric, Q[qi])[allow[qi]])
            radii[qi] = (d[19] + d[20]) / 2                    # 20 hits, none on the edge
            want_r.append(orc.search_exact(rows, dim, 32, metric, Q[qi], radius=float(radii[qi]), allow=m)[:2])
            want_k.append(orc.search_exact(rows, dim, 32, metric, Q[qi], k=k_big, allow=m)[:2])
        return rows, Q, allow, radii, want_r, want_k

    def radius_call(ix, c):
        rows, Q, allow, radii, want_r, _ = c
        got = ix.search_radius_batch(Q, radii, allow=allow)
        for qi in range(nq):
            assert len(want_r[qi][0]) == 20
            assert [int(x) for x in got[qi][0]] == [int(x) for x in want_r[qi][0]], ("radius", qi)
            assert (np.asarray(got[qi][1]) == want_r[qi][1]).all(), ("radius", qi)

    def topk_call(ix, c):
        rows, Q, allow, _, _, want_k = c
        r, d, cnt = ix.search_topk(Q, k_big, allow=allow)
        for qi in range(nq):
            assert cnt[qi] == len(want_k[qi][0]) == k_big
            assert [int(x) for x in r[qi]] == [int(x) for x in want_k[qi][0]], ("top-k", qi)
            assert (d[qi] == want_k[qi][1]).all(), ("top-k", qi)

    def open_index(**options):
        ix = ScanIndex(dim, 32, metric, devices=[0, 0])
        for name, value in dict({"multi_query": 0, "radius_mq": 0, "sketch_radius": 1, "sketch_topk_collect": 1},
                                **options).items():
            ix.set_option(name, value)
        return ix

    small = case(2005, 940 + metric)
    with open_index(sketch=1, sketch_min_rows=1) as ix:
        ix.load(small[0])
        ix.set_option("force_sketch_nomem", 1)
        for call in (lambda: ix.search_topk(small[1], 10), lambda: ix.search_topk(small[1], k_big),
                     lambda: ix.search_radius_batch(small[1], small[3])):
            with pytest.raises(Exception, match="force_sketch_nomem"):
                call()
        ix.set_option("sketch", 2)                             # auto mode: too few rows for a sketch, hook or no hook
        radius_call(ix, small)
        topk_call(ix, small)
        assert served_beyond_the_prepass(ix) == (0, 0)
        ix.set_option("sketch", 1)
        ix.set_option("force_sketch_nomem", 0)
        ix.load(small[0])
        radius_call(ix, small)
        topk_call(ix, small)
        if DEFAULT_TUNABLES:
            assert served_beyond_the_prepass(ix) == expected(2005)

    big = case(N, 950 + metric)
    with open_index(sketch=2) as ix:                           # automatic, as it is by default
        ix.set_option("force_sketch_nomem", 1)
        for call in (radius_call, topk_call):
            ix.load(big[0])                                    # (a load re-arms the sketch: each call meets the refusal itself)
            call(ix, big)                                      # no error: the full-precision path answers
            assert served_beyond_the_prepass(ix) == (0, 0)
        ix.set_option("force_sketch_nomem", 0)
        radius_call(ix, big)
        topk_call(ix, big)
        assert served_beyond_the_prepass(ix) == (0, 0)         # aside until the next load
        ix.load(big[0])
        radius_call(ix, big)
        topk_call(ix, big)
        if DEFAULT_TUNABLES:
            assert served_beyond_the_prepass(ix) == expected(N)
