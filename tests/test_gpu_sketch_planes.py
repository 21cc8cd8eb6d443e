"""Two query planes on the sketch sweep (option "sketch_planes") and resident row norms in the grouped one-sweep scan
(option "scan_norms"), DESIGN.md 4.5 item 7.

The answers are the oracle's and the full-precision path's, bit for bit, whatever the two options and the group size
are.  At a fixed plane count the keys must not move at all: the resident norm is the float the sweep would have summed,
and the two-plane key of a group is the float the kernel without groups computes on the all-zero h plane -- so the
answers AND the split (settled by the sketch, handed over) are identical across scan_norms and scan_group.  The floor
on the settled share keeps the comparison from passing by falling back.
"""
import functools

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import ScanIndex, SZG_COSINE, SZG_EUCLIDEAN

pytestmark = pytest.mark.gpu

N = 6007                      # no multiple of 16 or of a wave step; above the default sketch_min_rows
K = 10
N_QUERIES = (1, 2, 3, 16, 17)  # G = 1 on the zero-h image, G = 2, an idle slot, a full launch, a second launch of one
PLANES = (2, 3)
NORMS = (0, 1)
GROUPS = (0, 1, 4)
CASES = [(d, m) for d in (768, 384, 100) for m in (SZG_COSINE, SZG_EUCLIDEAN)]   # shape 4x12, shape 4x6, any-shape
CASE_IDS = ["%d-%s" % (d, "cos" if m == SZG_COSINE else "euc") for d, m in CASES]


@functools.lru_cache(maxsize=2)
def corpus(dim):
    rng = np.random.default_rng(3100 + dim)
    V = rng.standard_normal((N + 64, dim)).astype(np.float32).astype(np.float64)
    return V, rng.standard_normal((max(N_QUERIES), dim))


def oracle_answers(rows, dim, metric, Q, allow=None):
    a = None if allow is None else allow.astype(np.uint8)
    return [orc.search_exact(rows, dim, 32, metric, q, k=K, allow=a)[:2] for q in Q]


def assert_oracle(res, want, what):
    r, d, c = res
    for qi, (w_rows, w_dist) in enumerate(want):
        assert [int(x) for x in r[qi, : c[qi]]] == [int(x) for x in w_rows], ("rows differ", what, "query", qi)
        assert (np.asarray(d[qi, : c[qi]], dtype=np.float64) == np.asarray(w_dist, dtype=np.float64)).all(), \
            ("distances not bit-equal", what, "query", qi)


def same(a, b):
    return all((x == y).all() for x, y in zip(a, b))


def search(ix, Q, **opts):
    for name, v in opts.items():
        ix.set_option(name, v)
    ix.reset_stats()
    res = ix.search_topk(Q, K)
    return res, ix.stats()


@pytest.mark.parametrize("dim,metric", CASES, ids=CASE_IDS)
def test_planes_norms_groups(dim, metric):
    V, Qall = corpus(dim)
    rows = orc.encode_rows(V[:N], 32)
    want = oracle_answers(rows, dim, metric, Qall)
    with ScanIndex(dim, 32, metric) as ix:
        ix.load(rows)
        ix.set_option("multi_query", 0)
        for nq in N_QUERIES:
            Q = Qall[:nq]
            res, st = search(ix, Q, sketch=0)
            assert_oracle(res, want[:nq], ("sketch = 0", nq))
            assert st["sketch_queries"] + st["sketch_fallbacks"] == 0
            full = res
            ix.set_option("sketch", 1)
            for planes in PLANES:
                first = None
                for norms in NORMS:
                    for group in GROUPS:
                        what = ("queries", nq, "sketch_planes", planes, "scan_norms", norms, "scan_group", group)
                        res, st = search(ix, Q, sketch_planes=planes, scan_norms=norms, scan_group=group)
                        split = (st["sketch_queries"], st["sketch_fallbacks"])
                        print(what, "settled, handed over:", split)
                        assert_oracle(res, want[:nq], what)
                        assert same(res, full), what
                        assert sum(split) == nq and st["mq_queries"] == 0, (what, st)
                        if first is None:
                            first = (res, split)
                        assert same(res, first[0]) and split == first[1], (what, split, first[1])
            for planes in PLANES:   # the floor: the comparisons above were made on the sketch, not on the fallback
                res, st = search(ix, Q, sketch_planes=planes, scan_norms=0, scan_group=0)
                print("queries", nq, "sketch_planes", planes, "settled", st["sketch_queries"], "of", nq)
                if nq >= 16 and planes == 2:
                    assert 4 * st["sketch_queries"] >= 3 * nq, (nq, st["sketch_queries"])


def test_norm_bookkeeping():
    """The resident norms of the sketch rows follow the rows: appended rows, an overwritten row (a stale norm would
    move the key of the one row that has to win), a tombstone (masked launch: groups step aside), compact()."""
    dim, metric, nq = 768, SZG_COSINE, 16
    V, Qall = corpus(dim)
    V = V.copy()
    Q = Qall[:nq]
    n = N
    with ScanIndex(dim, 32, metric) as ix:
        for name, v in (("multi_query", 0), ("sketch", 1)):
            ix.set_option(name, v)
        ix.load(orc.encode_rows(V[:n], 32))
        rows = orc.encode_rows(V[:n], 32)
        res, st = search(ix, Q)
        assert_oracle(res, oracle_answers(rows, dim, metric, Q), "loaded")
        settled0 = st["sketch_queries"]
        # 1. rows added: norm_valid < n_rows, the norms catch up.  One of the new rows is (nearly) query 7 at ten times
        # the length: with a norm that was not computed it would not win, or the certificate would not hold
        r_app = n + 20
        V[r_app] = (10.0 * Q[7] + 1e-3 * V[r_app]).astype(np.float32).astype(np.float64)
        ix.append(orc.encode_rows(V[n : n + 37], 32))
        n += 37
        rows = orc.encode_rows(V[:n], 32)
        want = oracle_answers(rows, dim, metric, Q)
        assert int(want[7][0][0]) == r_app
        res, st = search(ix, Q)
        assert_oracle(res, want, "appended")
        assert int(res[0][7, 0]) == r_app
        assert st["sketch_queries"] + st["sketch_fallbacks"] == nq
        assert 4 * st["sketch_queries"] >= 3 * nq, st["sketch_queries"]
        # 2. one row overwritten with (nearly) query 3 at ten times the length: its norm changes a hundredfold
        r_new = 1234
        V[r_new] = (10.0 * Q[3] + 1e-3 * V[r_new]).astype(np.float32).astype(np.float64)
        ix.overwrite(r_new, orc.encode_rows(V[r_new : r_new + 1], 32))
        rows = orc.encode_rows(V[:n], 32)
        want = oracle_answers(rows, dim, metric, Q)
        assert int(want[3][0][0]) == r_new
        res, st = search(ix, Q)
        assert_oracle(res, want, "overwritten")
        assert int(res[0][3, 0]) == r_new
        assert 4 * st["sketch_queries"] >= 3 * nq, st["sketch_queries"]   # (a stale norm: the certificate fails or lies)
        # 3. a tombstone: the launch is masked
        live = np.ones(n, dtype=bool)
        dead = int(want[5][0][0])
        ix.tombstone(dead)
        live[dead] = False
        res, st = search(ix, Q)
        assert_oracle(res, oracle_answers(rows, dim, metric, Q, allow=live), "tombstoned")
        # 4. compact(): the norms are reset with the rows, groups are back
        ix.compact()
        rows = rows[live]
        res, st = search(ix, Q)
        assert_oracle(res, oracle_answers(rows, dim, metric, Q), "compacted")
        assert st["sketch_queries"] + st["sketch_fallbacks"] == nq
        print("settled: loaded", settled0, "compacted", st["sketch_queries"])


def test_plain_8bit_handle():
    """A plain 8-bit handle gets the resident norms (three planes stay): the same answers, the same scan_bytes -- row
    bytes only -- and the same escalations, launches and replays with scan_norms 0 and 1, and sketch_planes does not
    reach it.  (The norm is an exact integer sum converted once on either side; the library exposes no raw keys, so
    what a test can see of them is the certified path they take.)"""
    dim, n, nq = 768, 3000, 16
    rows = orc.synth_rows(3200, 0, n, dim, 8)
    Q = orc.synth_vectors(3201, 0, nq, dim)
    for metric in (SZG_COSINE, SZG_EUCLIDEAN):
        with ScanIndex(dim, 8, metric) as ix:
            ix.synth(n, 3200)
            for name, v in (("multi_query", 0), ("sketch", 0), ("scan_group", 0)):
                ix.set_option(name, v)
            got = {}
            for norms in NORMS:
                for planes in (0, 2):
                    res, st = search(ix, Q, scan_norms=norms, sketch_planes=planes)
                    got[norms, planes] = (res, st["scan_bytes"], (st["escalations"], st["scan_launches"], st["full_replays"]))
            want = [orc.search_exact(rows, dim, 8, metric, q, k=K)[:2] for q in Q]
            assert_oracle(got[0, 0][0], want, ("plain 8-bit", metric))
            for key, (res, swept, path) in got.items():
                assert same(res, got[0, 0][0]), key
                assert swept == got[0, 0][1] and swept % (n * rows.shape[1]) == 0, (key, swept)
                # these keys are certified: a key that moved would show as an escalation or a replay more or less
                assert path == got[0, 0][2], (key, path, got[0, 0][2])
            assert got[0, 0][1] < nq * n * rows.shape[1]   # (groups did serve: fewer passes than queries)
