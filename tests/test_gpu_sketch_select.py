"""The matrix sketch sweep's selection (kernels_scan_mx.hip; option sketch_select): lists of up to 16 entries are kept
as row lists -- list 4 c + r of a wave in the 16 lanes of lane-row c, register slot r, one candidate into each of the 16
per round -- where sketch_select = 1 keeps one whole-wave list per query and inserts one candidate at a time.

An insert is a set operation on unique entries, so both must leave the same lists bit for bit.  Per case the same call
runs under sketch_select 0 and 1 and everything the sweep hands on is compared byte for byte: the certificate trace's
sketch records (lb carries the drop bound) with their entries (rows, keys, bounds, distances), the answers and
szg_stats.scan_bytes.  Under the default the certificate chain (K_s, L_s, D, S) and the oracle's answers are checked as in
test_gpu_sketch_matrix.py.  sketch_list sets the list length m; m = 17 is the control: both settings take the serial
code there.

Block lists: up to 64 rows lie in one block (4 waves of 16 rows), so the merged list is that block's; one launch step
plus 77 rows spreads the rows over every block and the drop bound sees each block's m-th entry.
"""
import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import scan_select_plan
import test_gpu_sketch_matrix as tsm

pytestmark = pytest.mark.gpu

SEED = 0x53595A470000C000
EUC, COS = tsm.EUC, tsm.COS
MID = tsm.MID
REC_FIELDS = ("query", "pass_", "keys", "sweep", "certified", "k", "row_lo", "row_hi", "thr_min", "kmax", "thr", "eps",
              "D", "slack", "n_entries")   # (all but first_entry: where the record's entries lie in the trace)


def traced_call(ix, Q, k, what):
    """One top-k call -> (answers, scan_bytes, {query: (its sketch record's bytes, its entries' bytes)})"""
    ix.certificates()   # (records of earlier calls: read and dropped)
    ix.reset_stats()
    got = ix.search_topk(Q, k)
    st = ix.stats()
    recs, ents, dropped = ix.certificates()
    assert dropped == 0, what
    out = {}
    for r in recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]:
        q = int(r["query"])
        assert q not in out, ("two sketch records of one query", what, q)
        e = ents[int(r["first_entry"]): int(r["first_entry"]) + int(r["n_entries"])]
        out[q] = (b"".join(r[f].tobytes() for f in REC_FIELDS), e.tobytes(), r, e)
    assert sorted(out) == list(range(Q.shape[0])), ("one sketch record per query", what)
    return got, st["scan_bytes"], out


def assert_same_under_both(ix, Q, k, what):
    """The call under sketch_select 0 and 1: records, drop bound, entries, answers and scan_bytes byte for byte.
    -> the answers"""
    seen = {}
    for sel in (0, 1):
        ix.set_option("sketch_select", sel)
        seen[sel] = traced_call(ix, Q, k, what + ("sketch_select", sel))
    ix.set_option("sketch_select", 0)
    (g0, b0, t0), (g1, b1, t1) = seen[0], seen[1]
    for q in range(Q.shape[0]):
        r0, r1 = t0[q][2], t1[q][2]
        # (field by field first, for a message that says what moved)
        assert r0["thr_min"].tobytes() == r1["thr_min"].tobytes(), ("drop bound / lb differs", what, q, r0["thr_min"], r1["thr_min"])
        assert int(r0["n_entries"]) == int(r1["n_entries"]), ("entry counts differ", what, q)
        e0, e1 = t0[q][3], t1[q][3]
        assert (e0["row"] == e1["row"]).all(), ("rows differ", what, q, e0["row"], e1["row"])
        assert e0["key"].tobytes() == e1["key"].tobytes(), ("keys differ", what, q)
        assert t0[q][1] == t1[q][1], ("entries differ", what, q)
        assert t0[q][0] == t1[q][0], ("records differ", what, q, r0, r1)
    for a, b in zip(g0, g1):
        assert a.tobytes() == b.tobytes(), ("answers differ", what)
    assert b0 == b1, ("scan_bytes differ", what, b0, b1)
    return g0


# ---- the lattice ---------------------------------------------------------------------------------------------------
MS = (1, 2, 7, 8, 15, 16, 17)
ROWS = (15, 16, 17, 33, "s1")
NQS = (3, 16, 17)
DIMS = (64, 384, 768)   # the any-steps kernel and the two shaped ones


def lattice():
    """Every m with every kernel form; within a form every row count, query count and metric (7 cases each) -- and a
    second round at other offsets for the lengths at the lists' edges, so that the pairs of the other axes fill up."""
    out = []
    for d, dim in enumerate(DIMS):
        for i, m in enumerate(MS):
            out.append((dim, m, ROWS[(i + d) % 5], NQS[(i + 2 * d) % 3], (i + d) % 2))
        for i, m in enumerate((1, 8, 16)):
            out.append((dim, m, ROWS[(i + d + 3) % 5], NQS[(i + 2 * d + 1) % 3], (i + d + 1) % 2))
    return out


CASES = lattice()


def case_id(c):
    dim, m, rows, nq, metric = c
    return "d%d-m%d-n%s-q%d-%s" % (dim, m, rows, nq, MID[metric])


def test_lattice_covers_every_value_with_every_form():
    for dim in DIMS:
        mine = [c for c in CASES if c[0] == dim]
        assert {c[1] for c in mine} == set(MS) and {c[2] for c in mine} == set(ROWS), dim
        assert {c[3] for c in mine} == set(NQS) and {c[4] for c in mine} == {EUC, COS}, dim
    # which launches keep row lists: every launch of these calls is the matrix sweep's, lists of up to 16 under 0 only
    for nq in NQS:
        for n_l in tsm.launch_sizes(nq):
            for m in MS:
                assert scan_select_plan(64, 8, n_l, kp=m) == {"serves": True, "row_lists": m <= 16}
                assert scan_select_plan(64, 8, n_l, kp=m, sketch_select=1) == {"serves": True, "row_lists": False}


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_same_lists_under_both_selections(case):
    dim, m, rows, nq, metric = case
    k = 10
    assert m < tsm.sketch_kp(k)   # (short lists: sketch_list is the sweep's list length)
    n = tsm.n_rows_of(dim, rows)
    seed = SEED + dim * 100 + (n % 1000) + m
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    what = ("select", case_id(case), "rows", n)
    with tsm.open_sketched(dim, metric, sketch_list=m) as ix:
        ix.synth(n, seed)
        assert_same_under_both(ix, Q, k, what)
        # K_s, L_s with the drop bound, D, S and the oracle's answers, under the default
        got, st, checked, settled, _ = tsm.certified_call(ix, corpus, Q, k, what)
        assert st["sketch_queries"] + st["sketch_fallbacks"] == nq and st["mq_queries"] == 0, (what, st)
        tsm.assert_pass_count(st, n, dim, nq, tsm.matrix_passes(nq), what)
        print(what, "keys checked", checked, "settled", settled)


# ---- hand-made orders ----------------------------------------------------------------------------------------------
HAND_DIM, HAND_NQ = 64, 20   # 20 queries: launches of 16 (a whole group) and 4


def ladder(n, rng):
    """Unit rows at angles to the unit vector q that shrink with the row number, 0.45 pi down to 0.05 pi: for a query
    near q every row beats all before it; for a query near -q every row loses to all before it."""
    q = rng.standard_normal(HAND_DIM)
    q /= np.linalg.norm(q)
    V = np.zeros((n, HAND_DIM))
    for i in range(n):
        u = rng.standard_normal(HAND_DIM)
        u -= u.dot(q) * q
        u /= np.linalg.norm(u)
        a = np.pi * (0.45 - 0.4 * i / n)
        V[i] = np.cos(a) * q + np.sin(a) * u
    return V, q


def hand_case(order, n):
    """-> (rows float64[n, dim], queries [HAND_NQ, dim], near: the queries for which every row beats all before it)"""
    rng = np.random.default_rng(5200 + n)
    if order == "improving pairs":
        # every ladder row twice, the last one once: equal keys side by side, and better rows after them push entries
        # out of a full list -- which of two equal keys leaves is decided by the row half of the 64-bit compare alone,
        # and the odd row count leaves half a pair in the final list
        assert n % 2 == 1
        V, q = ladder((n + 1) // 2, rng)
        V = np.repeat(V, 2, axis=0)[:n]
    else:
        V, q = ladder(n, rng)
    jitter = 1e-3 * rng.standard_normal((HAND_NQ, HAND_DIM))
    if order in ("improving", "improving pairs"):   # 16 passing lanes per lane-row and tile: the most rounds
        near = set(range(HAND_NQ))
    elif order == "worsening":     # only the first m rows pass
        near = set()
    elif order == "identical":     # equal keys: (key, row) order decides, rows 0 .. m - 1 stay
        V[:] = V[n // 2]
        near = set()
    elif order == "one of a slot":     # query 5 = lane-row 1, slot 1; its slot's other lane-rows (1, 9, 13) are far
        near = {5}
    else:                              # "slots of a lane-row": of queries 8 .. 11 (lane-row 2) only 10 is near
        assert order == "slots of a lane-row"
        near = set(range(16)) - {8, 9, 11}
    Q = np.stack([(q if x in near else -q) + jitter[x] for x in range(HAND_NQ)])
    return V, Q, near


ORDERS = ("improving", "improving pairs", "worsening", "identical", "one of a slot", "slots of a lane-row")
HAND_ROWS = {"improving": 48, "improving pairs": 47, "worsening": 33, "identical": 16, "one of a slot": 48,
             "slots of a lane-row": 40}


@pytest.mark.parametrize("m", (1, 2, 8, 16))
@pytest.mark.parametrize("order", ORDERS, ids=[o.replace(" ", "_") for o in ORDERS])
def test_hand_made_orders(order, m):
    n, k = HAND_ROWS[order], 10
    V, Q, near = hand_case(order, n)
    V = V.astype(np.float32).astype(np.float64)
    packed = orc.encode_rows(V, 32)
    for metric in (COS, EUC):
        what = ("hand-made", order, "m", m, MID[metric], "rows", n)
        dists = np.stack([orc.all_distances(packed, HAND_DIM, 32, metric, q) for q in Q])
        if order == "improving pairs":
            for x in range(HAND_NQ):
                step = np.diff(dists[x])
                assert (step[0::2] == 0).all() and (step[1::2] < 0).all(), (what, x)
        elif order != "identical":   # the order the case is about holds in float64, query by query
            for x in range(HAND_NQ):
                step = np.diff(dists[x])
                assert (step < 0).all() if x in near else (step > 0).all(), (what, x)
        with tsm.open_sketched(HAND_DIM, metric, sketch_list=m) as ix:
            ix.load(packed)
            got = assert_same_under_both(ix, Q, k, what)
            tsm.assert_answers(got, packed, HAND_DIM, metric, Q, k, None, what)
