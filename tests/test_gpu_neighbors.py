"""szg_index_neighbors against the float64 oracle: entry i is the oracle's top-k for the decoded stored row q_i -- ids,
distances bit for bit, order and counts -- through the join kernel (every operand form: registers, LDS, query blocks of
64 and 32; masked and unmasked; both metrics) and through the masked search's route; and the join may not hide behind
that route: on rows without ties it hands over at most a quarter of what it tries.  The join is switched on through
szg_debug_join_min_queries: by default no call takes it, because it measured slower than the route."""
import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import Collection, CollectionOptions, ScanIndex, SearchArgs, SzgError, SZG_COSINE, SZG_EUCLIDEAN, _lib
from syzgydb_amd import cert_check as cc

pytestmark = pytest.mark.gpu

C, E = SZG_COSINE, SZG_EUCLIDEAN


def vectors(n, dim, seed, dup=False, zero=False):
    """Plain gaussian rows up to 192 dimensions; from 768 on gaussian clusters of about 20 rows.  scripts/neighbors_model.py
    (the certificate on the CPU, all rows as queries; profiles/neighbors.txt) says why: at these row counts plain rows of
    768 and more dimensions lie too evenly for ANY sketch certificate -- the model hands over 704 of 2 001 (768, cosine)
    to 1 022 of 1 025 (2 112) -- while it hands over 0 or 1 of the plain rows at 64 and 192 and none of the clustered ones.
    dup: every row twice (ties); zero: rows 5 and n - 1 all zero"""
    g = np.random.default_rng(seed)
    if dim <= 192:
        v = g.standard_normal((n, dim))
    else:
        centers = g.standard_normal((max(1, n // 20), dim))
        v = centers[np.arange(n) % centers.shape[0]] + 0.3 * g.standard_normal((n, dim))
    if dup:
        v[n // 2:] = v[: n - n // 2]
    if zero:
        v[5] = 0.0
        v[n - 1] = 0.0
    return v


# bits, metric, dim, rows, queries, as a list, k, what
CASES = [
    (32, C, 64, 16 * 70 - 1, 65, False, 10, ""),
    (32, E, 192, 16 * 70, 130, True, 1, ""),
    (32, C, 768, 16 * 125 + 1, 130, True, 10, ""),
    (32, E, 768, 16 * 125 + 1, 65, False, 10, ""),
    (32, E, 1088, 16 * 100 - 1, 65, False, 10, ""),       # 17 steps: the A operand in LDS
    (32, C, 2112, 16 * 64 + 1, 65, True, 10, ""),          # query blocks of 32
    (64, C, 192, 16 * 70, 65, False, 10, "f64"),
    (32, C, 192, 16 * 125, 130, True, 10, "mask"),         # ~5 % pass, a tombstoned row and query row, an empty tile
    (32, E, 192, 16 * 70, 65, False, 10, "mask"),
    (32, C, 64, 16 * 70, 65, False, 10, "dup"),            # ties fall back, the answers stay equal
    (32, C, 192, 16 * 70, 65, True, 10, "zero"),
    (32, E, 192, 16 * 140, 130, True, 10, "two"),          # two shards on one device
    (32, C, 64, 16 * 70 - 1, 1, False, 10, ""),            # one query: a partial tile, three idle waves, 70 slices
    (32, C, 768, 16 * 125 + 1, 16, True, 10, ""),
    (32, E, 64, 16 * 70 - 1, 17, False, 1, ""),
    (32, C, 2112, 16 * 64 + 1, 17, True, 10, ""),
    (32, E, 64, 16 * 70 - 1, 17, False, 1, "short"),       # below the threshold the hook sets (64): the route
    (16, C, 192, 16 * 70, 65, False, 10, "route"),
    (32, C, 192, 16 * 70, 65, False, 40, "route"),         # kp > 96
    (32, C, 192, 16 * 70, 65, False, 10, "default"),       # without the hook no call takes the join: it measured slower
]


@pytest.mark.parametrize("bits,metric,dim,n,nq,as_list,k,what", CASES)
def test_neighbors_match_the_oracle(bits, metric, dim, n, nq, as_list, k, what):
    g = np.random.default_rng(7)
    rows = orc.encode_rows(vectors(n, dim, 3, dup=what == "dup", zero=what == "zero"), bits)
    with ScanIndex(dim, bits, metric, devices=[0, 0] if what == "two" else None) as ix:
        ix.set_option("sketch", 1)
        ix.set_option("sketch_min_rows", 1)
        if what == "f64":
            ix.set_option("sketch_f64", 1)
        if what != "default":
            ix.debug_join_min_queries(64 if what == "short" else 1)
        ix.load(rows)
        allow = mask = None
        if what == "mask":
            allow = g.random(n) < 0.05
            allow[64:96] = False                  # tiles 4 and 5 hold no eligible row
            allow[[3, 40]] = True
            ix.tombstone(40)                      # an allowed row that is dead
            ix.tombstone(7)                       # ... and a dead row that is a query
            mask = ix.mask(allow)
        if as_list:
            q = g.permutation(n)[:nq].astype(np.uint64)
            q[-1] = q[0]                          # a duplicate
        else:
            q = np.arange(n - nq, n, dtype=np.uint64)
        if what == "mask":
            q[1] = 7
        if what == "zero":
            q[2] = 5
        ix.reset_stats()
        ix.trace_certificates(True)
        r, d, c = ix.neighbors(rows=q, k=k, mask=mask) if as_list or what in ("mask", "zero") else ix.neighbors(first=n - nq, n=nq, k=k)
        st = ix.neighbors_stats()
        recs, ents, dropped = ix.certificates()
        ix.trace_certificates(False)
        live = np.ones(n, dtype=bool)
        if what == "mask":
            live[[40, 7]] = False
        ok = (allow & live).astype(np.uint8) if allow is not None else None
        Q = np.stack([orc.decode_vector(rows[int(r_)], dim, bits) for r_ in q])
        joins = recs[recs["pass_"] == _lib.SZG_CERT_JOIN]
        if what not in ("short", "route", "default"):
            # every join record against float64: the sketch keys and their bound, the left-out rows, D, and 2 x slack
            assert len(joins) == nq
            info = ix.sketch_info()
            sketch = (cc.Corpus(ix.sketch_rows()[0], dim, 8, metric), info["gscale"], info["exc_rows"])
            dists = np.stack([orc.all_distances(rows, dim, bits, metric, x) for x in Q])
            elig = None if ok is None else ok.astype(bool)
            cc.check(cc.Corpus(rows, dim, bits, metric), Q, joins, ents, dropped, eligible=elig, dists=dists, sketch=sketch,
                     join_rows=q, what=(what, dim))
            assert (joins["slack"] == 2.0 * cc.sketch_slack(info["max_ang"], info["gscale"], dim)).all()
        else:
            assert len(joins) == 0
        for i in range(nq):
            query = Q[i]
            o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, metric, query, k=k, allow=ok)
            assert c[i] == len(o_rows)
            assert list(map(int, r[i, : c[i]])) == list(map(int, o_rows)), i
            od = np.asarray(o_dist, dtype=np.float64)
            assert ((d[i, : c[i]] == od) | (np.isnan(d[i, : c[i]]) & np.isnan(od))).all(), i
        assert st["queries"] == nq
        if what in ("short", "route", "default"):
            assert st["join_queries"] == 0
        else:
            assert st["join_queries"] == nq and st["join_launches"] >= 1
            print("join_fallbacks", st["join_fallbacks"], "of", nq)
            if what in ("", "f64", "two"):
                assert st["join_fallbacks"] <= st["join_queries"] // 4


def test_refusals_and_row_base():
    """Decided on the host before any launch: k < 1, a listed row or a range past the handle's rows (with and without a
    row base), a stale mask; n = 0 checks its arguments only."""
    dim, n = 64, 100
    rows = orc.encode_rows(vectors(n, dim, 5), 32)
    with ScanIndex(dim, 32, C) as ix:
        ix.load(rows)
        for kw, code in ((dict(rows=[0], k=0), _lib.SZG_E_INVALID), (dict(rows=[0], k=-1), _lib.SZG_E_INVALID),
                         (dict(rows=[3, n], k=1), _lib.SZG_E_RANGE), (dict(first=n - 1, n=2, k=1), _lib.SZG_E_RANGE),
                         (dict(first=n + 1, n=0, k=1), _lib.SZG_E_RANGE), (dict(first=n + 1, k=1), _lib.SZG_E_RANGE)):
            with pytest.raises(SzgError) as e:
                ix.neighbors(**kw)
            assert e.value.code == code, kw
        assert ix.neighbors(first=n, n=0, k=1)[0].shape == (0, 1)
        want = ix.neighbors(rows=[n - 1, 2], k=3)
        mask = ix.mask(np.ones(n, dtype=bool))
        ix.set_row_base(1000)
        got = ix.neighbors(rows=[1000 + n - 1, 1002], k=3, mask=mask)
        assert (got[0] == want[0] + 1000).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all()
        for kw in (dict(rows=[n - 1], k=1), dict(first=999, n=1, k=1), dict(first=1000 + n, n=1, k=1)):
            with pytest.raises(SzgError) as e:
                ix.neighbors(**kw)
            assert e.value.code == _lib.SZG_E_RANGE, kw
        ix.append(rows[:1])                       # the row count moves: the mask is stale
        with pytest.raises(SzgError) as e:
            ix.neighbors(rows=[1000], k=1, mask=mask)
        assert e.value.code == _lib.SZG_E_INVALID and "stale mask" in str(e.value)


def test_collection_neighbors():
    """By document id, through the Where mask; the document itself is a hit like any other."""
    from syzgydb_amd import where as W
    dim, n = 64, 200
    V = vectors(n, dim, 9)
    c = Collection(CollectionOptions(Name="nb", DistanceMethod=1, DimensionCount=dim, Quantization=32), devices=[0])
    try:
        ids = list(range(500, 500 + n))
        c.AddDocuments(ids, V, [b'{"n": %d}' % i for i in ids])
        c.IndexField("n", "number")
        where = W.Field("n") < 600
        ask = [650, 501, 650]
        for flt in (dict(), dict(Where=where)):
            got = c.Neighbors(ask, 4, **flt)
            for i, res in zip(ask, got):
                row = c._row_of[i]
                q = orc.decode_vector(c._index.read_rows(row, 1)[0], dim, 32)
                want = c.Search(SearchArgs(Vector=q, K=4, **flt))
                assert [r.ID for r in res.Results] == [r.ID for r in want.Results]
                a, b = (np.array([r.Distance for r in x.Results]) for x in (res, want))
                assert ((a == b) | (np.isnan(a) & np.isnan(b))).all()
            assert 501 in [r.ID for r in got[1].Results]          # (the document itself: the reference's own distance to it)
            assert (650 in [r.ID for r in got[0].Results]) == (not flt)
    finally:
        c.Close()
