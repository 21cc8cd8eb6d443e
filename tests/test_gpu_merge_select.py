"""The short-list merge of the sketch sweep by selection (merge_short_kernel): one block per query takes
the kp-th smallest of the block lists' first entries as a threshold h, compacts the entries <= h, sorts them with one
bitonic network and writes the kp best and the drop bound; when more entries are <= h than its buffer sorts at once
(64 g kp - 2 entries for g groups of 64 lists, rounded down to a power of two) it runs the tournament instead.  Entries
are unique 64-bit values, so the result is defined without reference to the method.

Reference: the same calls under sketch_list >= kp (full lists, the two-level merge, no drop bound).  Answers are the
same bit for bit in every case; where the drop bound does not lower the certificate's bound (thr_min equal on both
sides) the traced list is the same entry for entry.
"""
import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import ScanIndex, SZG_COSINE, SZG_EUCLIDEAN, _lib
from syzgydb_amd.index import merge_short_plan, scan_plan

pytestmark = pytest.mark.gpu

DIM = 64                       # tiled 8-bit sketch rows: 16 rows per wave, 64 per block
PLAN = scan_plan(DIM, 8, 1 << 22, kp=40)
ROWS_PER_BLOCK, FULL_GRID = PLAN["rows_per_block"], PLAN["grid"]
assert PLAN["tiled"] and ROWS_PER_BLOCK == 64
SHAPES = {"64-lists": 4096,                           # one group of lists: the buffer is shorter than kp -- the tournament
          "68-lists": 4096 + 3 * 64 + 4,              # no multiple of 64 lists, a last block whose lists are not full
          "full-grid": FULL_GRID * ROWS_PER_BLOCK * 2 + 77}
# (k, sketch_extra, sketch_list): kp = k + sketch_extra; the one-launch merge serves 1 <= m < kp <= 64
KPS = {"kp2-m1": (1, 1, 1), "kp40-auto": (10, 30, 0), "kp64-auto": (34, 30, 0), "kp64-m63": (10, 54, 63)}


def auto_m(kp, lists):
    """the automatic list length of a sketch sweep over `lists` blocks (sketch_list = 0)"""
    return max(8, 2 * kp // lists + 8)


def test_which_path_each_shape_takes():
    """merge_short_plan: the most entries under the threshold that the selection's network sorts.  Below kp the launch
    can only run the tournament; the shapes and list lengths here are chosen so that both paths are on record."""
    lists = {name: min(FULL_GRID, -(-n // ROWS_PER_BLOCK)) for name, n in SHAPES.items()}   # one list per block
    assert lists["64-lists"] == 64 and lists["68-lists"] == 68 and lists["full-grid"] == FULL_GRID >= 512
    # one group of lists: the buffer (kp - 2 words) never holds the kp entries a full result needs
    for kp in (2, 40, 64):
        m = 1 if kp == 2 else auto_m(kp, 64)
        p = merge_short_plan(64, m, kp)
        assert p["fits"] and p["sorts"] < kp, (kp, p)
    # two groups: 2 kp - 2 words, a network of 64 at kp = 40 and at kp = 64 (126 words)
    assert merge_short_plan(68, auto_m(40, 68), 40) == {"fits": True, "sorts": 64}
    assert merge_short_plan(68, auto_m(64, 68), 64) == {"fits": True, "sorts": 64}
    # the full grid: 8 groups and more -- random rows pass about kp + 2 entries, far inside the network
    g = -(-FULL_GRID // 64)
    full = merge_short_plan(FULL_GRID, 8, 40)
    assert full["fits"] and full["sorts"] >= 256 and full["sorts"] <= g * 40 - 2
    assert merge_short_plan(FULL_GRID, 8, 64)["sorts"] >= 256
    assert not merge_short_plan(FULL_GRID, 63, 64)["fits"]      # (kp64-m63 there: full lists, the two-level merge)
    assert merge_short_plan(64, 63, 64)["fits"]


def open_index(V, metric):
    ix = ScanIndex(V.shape[1], 32, metric)
    ix.load(orc.encode_rows(V, 32))
    for name, v in (("multi_query", 0), ("sketch", 1), ("sketch_min_rows", 1)):
        ix.set_option(name, v)
    ix.trace_certificates(True)
    return ix


def search_both(ix, Q, k, extra, lst):
    """-> {mode: (rows, dists, counts, stats, records, entries)} for the short lists and the full ones"""
    out = {}
    ix.set_option("sketch_extra", extra)
    for mode, m in (("short", lst), ("full", 4096)):
        ix.set_option("sketch_list", m)
        ix.reset_stats()
        r, d, c = ix.search_topk(Q, k)
        recs, ents, dropped = ix.certificates()
        assert dropped == 0
        out[mode] = (r, d, c, ix.stats(), recs, ents)
    return out


def compare(res, what, lists=True):
    """answers bit for bit; lists: the sketch's traced list entry for entry where the drop bound did not lower thr_min
    (rows with distinct keys: a bound that ties with the kp-th key leaves thr_min where it was and still drops rows).
    -> queries whose lists were compared"""
    (rs, ds, cs, _, recs_s, ents_s), (rf, df, cf, _, recs_f, ents_f) = res["short"], res["full"]
    assert (cs == cf).all(), what
    for qi in range(len(cs)):
        n = cs[qi]
        assert (rs[qi, :n] == rf[qi, :n]).all(), (what, qi)
        assert (ds[qi, :n].view(np.uint64) == df[qi, :n].view(np.uint64)).all(), (what, qi)
    compared = 0
    sk_s = recs_s[recs_s["pass_"] == _lib.SZG_CERT_SKETCH]
    sk_f = recs_f[recs_f["pass_"] == _lib.SZG_CERT_SKETCH]
    assert len(sk_s) == len(sk_f) == len(cs), what
    for a in sk_s:
        b = sk_f[sk_f["query"] == a["query"]][0]
        same_bound = a["thr_min"] == b["thr_min"] or (np.isnan(a["thr_min"]) and np.isnan(b["thr_min"]))
        if not same_bound:
            assert a["thr_min"] < b["thr_min"], (what, "the drop bound can only lower the bound")
            continue
        if not lists:
            continue
        ea = ents_s[int(a["first_entry"]): int(a["first_entry"] + a["n_entries"])]
        eb = ents_f[int(b["first_entry"]): int(b["first_entry"] + b["n_entries"])]
        assert ea.tobytes() == eb.tobytes(), (what, "query", int(a["query"]), "merged lists differ")
        compared += 1
    return compared


def oracle_check(V, metric, Q, k, res, what):
    rows = orc.encode_rows(V, 32)
    r, d, c = res["short"][:3]
    for qi in range(Q.shape[0]):
        o_rows, o_dist, _ = orc.search_exact(rows, V.shape[1], 32, metric, Q[qi], k=k)
        assert [int(x) for x in r[qi, : c[qi]]] == [int(x) for x in o_rows], (what, qi)
        assert (d[qi, : c[qi]] == o_dist).all(), (what, qi)


@pytest.mark.parametrize("metric", [SZG_COSINE, SZG_EUCLIDEAN], ids=["cos", "euc"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_random_rows_every_kp(shape, metric):
    """Random rows: the shortest and the longest kp the one-launch merge serves, automatic and explicit list lengths."""
    n = SHAPES[shape]
    rng = np.random.default_rng(7100 + n % 1000 + metric)
    V = rng.standard_normal((n, DIM))
    Q = rng.standard_normal((5, DIM))
    compared = 0
    with open_index(V, metric) as ix:
        for name, (k, extra, lst) in KPS.items():
            res = search_both(ix, Q, k, extra, lst)
            compared += compare(res, (shape, name))
            if name == "kp40-auto":
                oracle_check(V, metric, Q, k, res, (shape, name))
                st = res["short"][3]
                assert st["sketch_queries"] + st["sketch_fallbacks"] == Q.shape[0], st
    assert compared > 0, "no query whose merged list could be compared"


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_duplicate_rows_order_by_row(shape):
    """Every fourth row is one of three vectors near the query: equal keys, ordered by their rows, across many lists.
    (Every block holds more of them than a short list keeps: the lists differ from the full ones by construction, the
    answers must not.)"""
    n = SHAPES[shape]
    rng = np.random.default_rng(7200 + n % 1000)
    V = rng.standard_normal((n, DIM))
    q = rng.standard_normal(DIM)
    near = [q + 0.05 * rng.standard_normal(DIM) for _ in range(3)]
    for i in range(0, n, 4):
        V[i] = near[(i // 4) % 3]
    Q = np.stack([q, 2.0 * q, near[0]])
    with open_index(V, SZG_COSINE) as ix:
        for name in ("kp40-auto", "kp64-auto"):
            k, extra, lst = KPS[name]
            res = search_both(ix, Q, k, extra, lst)
            compare(res, (shape, name, "duplicates"), lists=False)
            if name == "kp40-auto":
                oracle_check(V, SZG_COSINE, Q, k, res, (shape, "duplicates"))


def close_rows(V, q, rng, rows, first_angle, step):
    """rows[i] at angular distance first_angle + i * step from q"""
    for i, r in enumerate(rows):
        u = rng.standard_normal(V.shape[1])
        u -= u.dot(q) * q
        u /= np.linalg.norm(u)
        a = np.pi * (first_angle + step * i)
        V[r] = np.cos(a) * q + np.sin(a) * u


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_drop_bound_binds(shape):
    """One block holds 40 of the query's best rows, more than a short list keeps: the drop bound binds, sketch_fallbacks
    counts it and the answers are those of the full lists."""
    n = SHAPES[shape]
    rng = np.random.default_rng(7300 + n % 1000)
    V = rng.standard_normal((n, DIM))
    q = rng.standard_normal(DIM)
    q /= np.linalg.norm(q)
    close_rows(V, q, rng, range(40), 0.02, 0.001)
    Q = np.stack([q, q * 2.0, q + 1e-4 * np.arange(DIM) / DIM])
    k, extra, lst = KPS["kp40-auto"]
    with open_index(V, SZG_COSINE) as ix:
        res = search_both(ix, Q, k, extra, lst)
        compare(res, (shape, "crowded block"))
        oracle_check(V, SZG_COSINE, Q, k, res, (shape, "crowded block"))
        assert [int(x) for x in res["short"][0][0]] == list(range(k))
        assert res["full"][3]["sketch_queries"] == Q.shape[0]        # full lists: settled
        assert res["short"][3]["sketch_queries"] == 0                # short lists: the drop bound binds ...
        assert res["short"][3]["sketch_fallbacks"] == Q.shape[0]     # ... and every query takes the full sweep


def test_more_entries_under_the_threshold_than_the_network_sorts():
    """Full grid, kp = 40, lists of 8: the query's 384 best rows sit eight to a block in 48 blocks, block b holding ranks
    8 b .. 8 b + 7.  The 40th smallest first entry is rank 312, so about 313 entries are <= h -- more than the 256 the
    network sorts in a buffer of 8 * 40 - 2 entries: the tournament runs.  (Block 0's eighth row is the drop bound, under
    the k-th distance: the queries fall back, with the exact answers.)  A second query far from the planted rows finds
    few entries <= h and goes through the network on the same corpus."""
    n = SHAPES["full-grid"]
    rng = np.random.default_rng(7400)
    V = rng.standard_normal((n, DIM))
    q = rng.standard_normal(DIM)
    q /= np.linalg.norm(q)
    blocks = rng.choice(FULL_GRID, size=48, replace=False)
    # (the launch's first step: block b holds rows [64 b, 64 b + 64))
    rows = [int(b) * ROWS_PER_BLOCK + 8 * i for b in blocks for i in range(8)]
    close_rows(V, q, rng, rows, 0.02, 0.0004)
    Q = np.stack([q, -q + 0.3 * rng.standard_normal(DIM)])
    k, extra, lst = KPS["kp40-auto"]
    # at least 8 * 39 + 1 planted entries are at or under the 40th smallest first entry: beyond the network
    assert merge_short_plan(FULL_GRID, 8, k + extra)["sorts"] < 8 * 39 + 1 <= 8 * 48
    with open_index(V, SZG_COSINE) as ix:
        ix.set_option("sketch_list", 8)
        res = search_both(ix, Q, k, extra, 8)
        compare(res, ("tournament",))
        oracle_check(V, SZG_COSINE, Q, k, res, ("tournament",))
        assert [int(x) for x in res["short"][0][0]] == rows[:k]
        assert res["short"][3]["sketch_fallbacks"] >= 1
