"""Short per-block lists in the sketch sweep (option "sketch_list"): the sweep keeps m < kp candidates
per wave and per block, one merge launch selects the kp best and the drop bound, and the certificate takes the lower
of the two.  Answers are those of the full lists (sketch_list >= kp) and of the full sweep (sketch=0), bit for bit."""
import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import ScanIndex, SZG_COSINE, SZG_EUCLIDEAN

pytestmark = pytest.mark.gpu
N = 65536
MODES = (("auto", {"sketch": 1, "sketch_list": 0}),
         ("full", {"sketch": 1, "sketch_list": 4096}),   # >= kp: the full lists and the two-level merge
         ("off", {"sketch": 0}))


def oracle_check(rows, dim, metric, Q, k, r, d, c, mask=None):
    for qi in range(Q.shape[0]):
        o_rows, o_dist, _ = orc.search_exact(rows, dim, 32, metric, Q[qi], k=k, allow=mask)
        assert c[qi] == len(o_rows), qi
        assert [int(x) for x in r[qi, : c[qi]]] == [int(x) for x in o_rows], qi
        got = d[qi, : c[qi]]
        assert ((got == o_dist) | (np.isnan(got) & np.isnan(o_dist))).all(), qi


def run_modes(ix, Q, k, allow=None):
    """{mode: (rows, dists, counts, settled by the sketch, handed over)} -- the same queries under each mode"""
    kw = {} if allow is None else {"allow": np.tile(allow, (Q.shape[0], 1))}
    out = {}
    for name, opts in MODES:
        for o, v in opts.items():
            ix.set_option(o, v)
        ix.reset_stats()
        r, d, c = ix.search_topk(Q, k, **kw)
        st = ix.stats()
        out[name] = (r, d, c, st["sketch_queries"], st["sketch_fallbacks"])
    return out


def same_answers(res):
    ra, da, ca = res["auto"][:3]
    for name in ("full", "off"):
        r, d, c = res[name][:3]
        assert (c == ca).all(), name
        for qi in range(len(c)):
            n = c[qi]
            assert (r[qi, :n] == ra[qi, :n]).all(), (name, qi)
            assert (d[qi, :n].view(np.uint64) == da[qi, :n].view(np.uint64)).all(), (name, qi)


@pytest.mark.parametrize("metric", [SZG_COSINE, SZG_EUCLIDEAN])
@pytest.mark.parametrize("k", [1, 10, 34])
def test_short_lists_answer_what_full_lists_answer(metric, k):
    dim = 48
    rng = np.random.default_rng(1200 + k + 7 * metric)
    n = N + 4000
    V = rng.standard_normal((n, dim))
    rows = orc.encode_rows(V, 32)
    Q = rng.standard_normal((6, dim))
    allow = rng.random(n) < 0.7
    for devices in (None, [0, 0]):
        kw = {} if devices is None else {"devices": devices}
        with ScanIndex(dim, 32, metric, **kw) as ix:
            ix.load(rows)
            ix.set_option("multi_query", 0)
            res = run_modes(ix, Q, k)
            same_answers(res)
            oracle_check(rows, dim, metric, Q, k, *res["auto"][:3])
            assert res["auto"][3] == res["full"][3] >= 4      # random data: the short lists settle as much
            live = np.ones(n, bool)
            for r0 in (5, 70, 30000, n - 2):
                ix.tombstone(r0)
                live[r0] = False
            res = run_modes(ix, Q, k, allow=allow)
            same_answers(res)
            oracle_check(rows, dim, metric, Q, k, *res["auto"][:3], mask=(allow & live).astype(np.uint8))
            assert res["auto"][3] == res["full"][3]


@pytest.mark.parametrize("metric", [SZG_COSINE, SZG_EUCLIDEAN])
def test_small_forced_handle(metric):
    """4 096 rows, sketch forced on: few blocks, so the automatic lists are longer per block."""
    dim = 64
    rng = np.random.default_rng(1300 + metric)
    V = rng.standard_normal((4096, dim))
    rows = orc.encode_rows(V, 32)
    Q = rng.standard_normal((5, dim))
    with ScanIndex(dim, 32, metric) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        for k in (1, 10, 34):
            res = run_modes(ix, Q, k)
            same_answers(res)
            oracle_check(rows, dim, metric, Q, k, *res["auto"][:3])
            assert res["auto"][3] == res["full"][3]
            assert res["auto"][3] + res["auto"][4] == Q.shape[0]


def crowded_block(seed, dim, n_close=40):
    """Random rows, except rows [0, n_close) -- all in the sweep's first block (16 rows per wave, 4 waves) -- at
    distinct angular distances 0.02, 0.021, ... from the query q"""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((N, dim))
    q = rng.standard_normal(dim)
    q /= np.linalg.norm(q)
    for i in range(n_close):
        u = rng.standard_normal(dim)
        u -= u.dot(q) * q
        u /= np.linalg.norm(u)
        a = np.pi * (0.02 + 0.001 * i)
        V[i] = np.cos(a) * q + np.sin(a) * u
    return V, q


def test_drop_bound_binds_and_answers_stay_exact():
    """One block holds 40 of the query's best rows, more than a short list keeps: the drop bound (the block's m-th
    entry) is then below the k-th distance and the query falls back to the full sweep, with the exact answer; the
    same corpus with the full lists settles through the sketch."""
    dim = 48
    V, q = crowded_block(1400, dim)
    rows = orc.encode_rows(V, 32)
    Q = np.stack([q, q * 2.0, q + 1e-4 * np.arange(dim) / dim])
    k = 10
    with ScanIndex(dim, 32, SZG_COSINE) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        res = run_modes(ix, Q, k)
        same_answers(res)
        oracle_check(rows, dim, SZG_COSINE, Q, k, *res["auto"][:3])
        assert [int(x) for x in res["auto"][0][0]] == list(range(k))
        assert res["full"][3] == Q.shape[0]            # full lists: settled
        assert res["auto"][3] == 0                     # short lists: the drop bound binds ...
        assert res["auto"][4] == Q.shape[0]            # ... and every query takes the full sweep


def test_mutations_between_searches():
    dim = 64
    rng = np.random.default_rng(1500)
    n = N + 2048
    V = rng.standard_normal((n + 3000, dim))
    R = orc.encode_rows(V, 32)
    Q = rng.standard_normal((6, dim))
    for devices in (None, [0, 0]):
        kw = {} if devices is None else {"devices": devices}
        with ScanIndex(dim, 32, SZG_COSINE, **kw) as ix:
            rows = R.copy()
            ix.load(rows[:n])
            ix.set_option("multi_query", 0)
            same_answers(run_modes(ix, Q, 10))
            ix.append(rows[n:])
            res = run_modes(ix, Q, 10)
            same_answers(res)
            oracle_check(rows, dim, SZG_COSINE, Q, 10, *res["auto"][:3])
            for r0 in (3, n - 7, n + 2900):                # overwrites: rows pulled next to query 1
                v = Q[1] * 2.0 + rng.standard_normal(dim) * 0.02
                rows[r0] = orc.encode_rows(v.reshape(1, -1), 32)[0]
                ix.overwrite(r0, rows[r0])
            res = run_modes(ix, Q, 10)
            same_answers(res)
            oracle_check(rows, dim, SZG_COSINE, Q, 10, *res["auto"][:3])
            live = np.ones(n + 3000, bool)
            for r0 in (3, 900, n + 1):
                ix.tombstone(r0)
                live[r0] = False
            res = run_modes(ix, Q, 10)
            same_answers(res)
            oracle_check(rows, dim, SZG_COSINE, Q, 10, *res["auto"][:3], mask=live.astype(np.uint8))
            assert res["auto"][3] > 0


def test_option_range():
    with ScanIndex(16, 32, SZG_COSINE) as ix:
        ix.set_option("sketch_list", 0)
        ix.set_option("sketch_list", 96)
        with pytest.raises(Exception):
            ix.set_option("sketch_list", -1)
