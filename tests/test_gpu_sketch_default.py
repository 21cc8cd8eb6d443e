"""The sketch pre-pass as the default ("sketch" option 2, automatic): float32 handles of >= 65 536 rows answer
one-query-per-sweep searches through the 8-bit sketch, step aside where it does not pay or does not fit, and
answer exactly what the reference loop answers either way."""
import os

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import ScanIndex, SZG_COSINE, SZG_EUCLIDEAN

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
