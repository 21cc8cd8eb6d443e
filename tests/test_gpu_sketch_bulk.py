"""The row lists' whole-tile merge (kernels_scan_mx.hip, RowList::merge_tile; option sketch_bulk): a tile of the matrix
sketch sweep whose pre-filter lets many (query, row) pairs of a wave through merges every list with its 16 candidates
whole, by a fixed sorting network in the lane-row, where the rounds insert one candidate per list and round.

An insert is a set operation on unique entries, so both must leave the same lists bit for bit.  Per case the same call
runs under sketch_bulk 1 (rounds only), 2 (every tile that selects at all is merged whole) and 0 (automatic) and everything
the sweep hands on is compared byte for byte with the run under 1: the certificate trace's sketch records (thr_min carries
the drop bound) with their entries, the answers and szg_stats.scan_bytes.  Under the default the certificate chain (K_s,
L_s, D, S) and the oracle's answers are checked as in test_gpu_sketch_matrix.py.

Lists of 17 entries take the serial inserts, where the option is inert: the control.  A wave meets more than one tile only from one
launch step of rows on ("s1", "s3": two to four tiles), so merges into non-empty and into full lists need those row
counts; the hand-made orders put their rows into the tiles ONE wave visits (t, t + S, t + 2 S; S the tiles of a step).
"""
import functools

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import scan_plan, scan_select_plan, scan_wide_plan
import test_gpu_sketch_matrix as tsm
import test_gpu_sketch_select as tss
import test_gpu_sketch_wide as tsw

pytestmark = pytest.mark.gpu

SEED = 0x53595A470000E000
EUC, COS = tsm.EUC, tsm.COS
MID = tsm.MID


def assert_same_under_bulk(ix, Q, k, what, values=(2, 0)):
    """The call under sketch_bulk 1 and under each of `values`: records, drop bound, entries, answers and scan_bytes byte
    for byte.  -> the answers"""
    ix.set_option("sketch_bulk", 1)
    g1, b1, t1 = tss.traced_call(ix, Q, k, what + ("sketch_bulk", 1))
    for v in values:
        ix.set_option("sketch_bulk", v)
        gv, bv, tv = tss.traced_call(ix, Q, k, what + ("sketch_bulk", v))
        for q in range(Q.shape[0]):
            r1, rv = t1[q][2], tv[q][2]
            # (field by field first, for a message that says what moved)
            assert r1["thr_min"].tobytes() == rv["thr_min"].tobytes(), ("drop bound / lb differs", what, v, q, r1["thr_min"], rv["thr_min"])
            assert int(r1["n_entries"]) == int(rv["n_entries"]), ("entry counts differ", what, v, q)
            e1, ev = t1[q][3], tv[q][3]
            assert (e1["row"] == ev["row"]).all(), ("rows differ", what, v, q, e1["row"], ev["row"])
            assert e1["key"].tobytes() == ev["key"].tobytes(), ("keys differ", what, v, q)
            assert t1[q][1] == tv[q][1], ("entries differ", what, v, q)
            assert t1[q][0] == tv[q][0], ("records differ", what, v, q, r1, rv)
        for a, b in zip(g1, gv):
            assert a.tobytes() == b.tobytes(), ("answers differ", what, v)
        assert b1 == bv, ("scan_bytes differ", what, v, b1, bv)
    ix.set_option("sketch_bulk", 0)
    return g1


# ---- the lattice ---------------------------------------------------------------------------------------------------
MS = (1, 2, 7, 8, 15, 16, 17)
ROWS = (15, 16, 17, 33, "s1", "s3")
# (queries, sketch_wide): one block of 16 queries per row read, and two (idle columns at 17 and 31, a second group at 33)
NQS = ((3, 0), (16, 0), (17, 0), (17, 2), (31, 2), (32, 2), (33, 2))
DIMS = (64, 384, 768)   # the any-steps kernel and the two shaped ones


def lattice():
    """Every m with every kernel form; within a form every row count, query count and metric (7 cases each) -- and a
    second round at other offsets for the lengths at the lists' edges, so that the pairs of the other axes fill up, on the
    row counts at which a wave meets several tiles."""
    out = []
    for d, dim in enumerate(DIMS):
        for i, m in enumerate(MS):
            out.append((dim, m, ROWS[(i + d) % 6], NQS[(i + 2 * d) % 7], (i + d) % 2))
        for i, m in enumerate((1, 8, 16)):
            out.append((dim, m, ("s3", "s1", "s3")[(i + d) % 3], NQS[(2 * i + d + 3) % 7], (i + d + 1) % 2))
    return out


CASES = lattice()


def case_id(c):
    dim, m, rows, (nq, wide), metric = c
    return "d%d-m%d-n%s-q%d-w%d-%s" % (dim, m, rows, nq, wide, MID[metric])


def test_lattice_covers_every_value_with_every_form():
    for dim in DIMS:
        mine = [c for c in CASES if c[0] == dim]
        assert {c[1] for c in mine} == set(MS) and {c[2] for c in mine} == set(ROWS), dim
        assert {c[3] for c in mine} == set(NQS) and {c[4] for c in mine} == {EUC, COS}, dim
        several = [c for c in mine if c[2] in ("s1", "s3") and c[1] <= 16]   # merges into lists that hold entries
        assert {c[3][1] for c in several} == {0, 2}, dim
    for m in MS:   # row lists up to 16 entries: the merge's kernels; 17 takes the serial inserts
        assert scan_select_plan(768, 8, 16, kp=m) == {"serves": True, "row_lists": m <= 16}
    assert scan_wide_plan(768, 8, 32, kp=15, sketch_wide=2)["serves"] and scan_wide_plan(384, 8, 32, kp=16, sketch_wide=2)["serves"]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_same_lists_under_every_value(case):
    dim, m, rows, (nq, wide), metric = case
    k = 10
    assert m < tsm.sketch_kp(k)   # (short lists: sketch_list is the sweep's list length)
    n = tsm.n_rows_of(dim, rows)
    seed = SEED + dim * 100 + (n % 1000) + m
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    what = ("bulk", case_id(case), "rows", n)
    with tsm.open_sketched(dim, metric, sketch_list=m, sketch_wide=wide) as ix:
        ix.synth(n, seed)
        assert_same_under_bulk(ix, Q, k, what)
        # K_s, L_s with the drop bound, D, S and the oracle's answers, under the default
        got, st, checked, settled, _ = tsm.certified_call(ix, corpus, Q, k, what)
        assert st["sketch_queries"] + st["sketch_fallbacks"] == nq and st["mq_queries"] == 0, (what, st)
        serves_wide = wide == 2 and tsw.wide_serves(dim, n, k, m)
        tsm.assert_pass_count(st, n, dim, nq, tsw.forced_passes(nq) if serves_wide else tsm.matrix_passes(nq), what)
        print(what, "keys checked", checked, "settled", settled)


# ---- the threshold's edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (64, 384))
def test_threshold_edges(dim):
    """Every threshold leaves the lists of sketch_bulk = 1: 2 and 3 (any tile that selects), 16 and 17 (one full slot of a
    lane-row), 511 and 512 (a two-block tile has at most 512 pairs: 512 needs every pair, 1 024 is never) and automatic."""
    n, nq, k, metric = tsm.n_rows_of(dim, "s3"), 32, 10, COS
    seed = SEED + 77 + dim
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    with tsm.open_sketched(dim, metric, sketch_list=8, sketch_wide=2) as ix:
        ix.synth(n, seed)
        assert_same_under_bulk(ix, Q, k, ("threshold edges", dim, "rows", n), values=(2, 3, 16, 17, 511, 512, 1024, 0))


# ---- hand-made orders --------------------------------------------------------------------------------------------------
HAND_DIM = 384
HAND_TILE = 5           # t: the first of the three tiles one wave visits


@functools.lru_cache(maxsize=1)
def hand_ground():
    """-> (S: tiles of a launch step, n rows, q, p: orthogonal unit vectors, the filler rows float32[n, dim]: all of them
    near -(q + p) / sqrt 2, far from every query of these cases under both metrics)"""
    S = tsm.rows_per_step(HAND_DIM) // 16
    n = (HAND_TILE + 2 * S) * 16 + 16
    assert scan_plan(HAND_DIM, 8, n, kp=8)["grid"] * 4 == S   # (a full grid: tile t's wave goes on to t + S and t + 2 S)
    rng = np.random.default_rng(7300)
    q = rng.standard_normal(HAND_DIM)
    q /= np.linalg.norm(q)
    p = rng.standard_normal(HAND_DIM)
    p -= p.dot(q) * q
    p /= np.linalg.norm(p)
    far = (-(q + p) / np.sqrt(2.0)).astype(np.float32)
    fill = far[None, :] + (0.004 * rng.standard_normal((n, HAND_DIM), dtype=np.float32))
    return S, n, q, p, fill


def hand_ladder(count, q, rng):
    """Unit rows at angles to q that shrink with the row number, 0.45 pi down to 0.05 pi: for a query near q every row
    beats all before it."""
    V = np.zeros((count, HAND_DIM))
    for i in range(count):
        u = rng.standard_normal(HAND_DIM)
        u -= u.dot(q) * q
        u /= np.linalg.norm(u)
        a = np.pi * (0.45 - 0.4 * i / count)
        V[i] = np.cos(a) * q + np.sin(a) * u
    return V


ORDERS = ("improving", "improving pairs", "worsening", "identical twice", "better tile worsening inside", "ties of the worst",
          "fifteen then a full tile", "alone in a second-block slot")


def hand_case(order, m, nq):
    """-> (rows float32[n, dim], queries float64[nq, dim], near: the queries that look at q; the others look at p)"""
    S, n, q, p, fill = hand_ground()
    rng = np.random.default_rng(7400 + len(order))
    L = hand_ladder(48, q, rng)
    tiles = [None, None, None]   # the 16 rows of tiles t, t + S, t + 2 S (None: filler)
    near = set(range(nq))
    if order == "improving":                       # 16 passing lanes per lane-row in each of the three tiles
        tiles = [L[0:16], L[16:32], L[32:48]]
    elif order == "improving pairs":               # equal keys side by side: the row half of the compare decides
        P = np.repeat(L[0::2], 2, axis=0)
        tiles = [P[0:16], P[16:32], P[32:48]]
    elif order == "worsening":                     # the first tile fills the lists, nothing after it enters
        R = L[::-1]
        tiles = [R[0:16], R[16:32], R[32:48]]
    elif order == "identical twice":               # 16 equal rows, and 16 more that equal the entries already listed
        tiles = [np.repeat(L[20:21], 16, axis=0), np.repeat(L[20:21], 16, axis=0), None]
    elif order == "better tile worsening inside":  # every row of the second and third tile beats a full list
        tiles = [L[0:16][::-1], L[16:32][::-1], L[32:48][::-1]]
    elif order == "ties of the worst":             # pass the float pre-filter, fail the exact compare (larger rows)
        tiles = [L[0:16], np.repeat(L[16 - m: 17 - m], 16, axis=0), L[32:48]]
    elif order == "fifteen then a full tile":      # 15 candidates and one far row, then 16 that all beat them
        tiles = [L[0:16].copy(), L[16:32], None]
        tiles[0][15] = fill[0]
    else:                                          # query 21 = second block, lane-row 1, slot 1
        assert order == "alone in a second-block slot" and nq > 21
        tiles = [L[0:16], L[16:32], L[32:48]]
        near = {21}
    V = fill.copy()
    for i, rows in enumerate(tiles):
        if rows is not None:
            r0 = (HAND_TILE + i * S) * 16
            V[r0: r0 + 16] = rows.astype(np.float32)
    jitter = 1e-3 * rng.standard_normal((nq, HAND_DIM))
    Q = np.stack([(q if x in near else p) + jitter[x] for x in range(nq)])
    return V, Q, near


HAND = [(o, m, (20, 0) if (i + j) % 2 else (32, 2)) for i, o in enumerate(ORDERS) for j, m in enumerate((1, 2, 8, 16))]
HAND = [(o, m, (32, 2) if o == "alone in a second-block slot" else nqw) for o, m, nqw in HAND]


@pytest.mark.parametrize("order,m,nqw", HAND, ids=["%s-m%d-q%d" % (o.replace(" ", "_"), m, nqw[0]) for o, m, nqw in HAND])
def test_hand_made_orders(order, m, nqw):
    (nq, wide), k = nqw, 10
    S, n, q, p, fill = hand_ground()
    V, Q, near = hand_case(order, m, nq)
    packed = orc.encode_rows(V.astype(np.float64), 32)
    metric = (COS, EUC)[(ORDERS.index(order) + m) % 2]
    what = ("hand-made", order, "m", m, "queries", nq, MID[metric], "rows", n)
    if order in ("improving", "worsening", "better tile worsening inside"):   # the order holds in float64
        rows = np.concatenate([np.arange(16) + (HAND_TILE + i * S) * 16 for i in range(3)])
        sub = orc.encode_rows(V[rows].astype(np.float64), 32)
        for x in sorted(near)[:4]:
            d = orc.all_distances(sub, HAND_DIM, 32, metric, Q[x])
            if order == "improving":
                assert (np.diff(d) < 0).all(), (what, x)
            elif order == "worsening":
                assert (np.diff(d) > 0).all(), (what, x)
            else:
                assert d[16:32].max() < d[0:16].min() and d[32:48].max() < d[16:32].min(), (what, x)
    with tsm.open_sketched(HAND_DIM, metric, sketch_list=m, sketch_wide=wide) as ix:
        ix.load(packed)
        got = assert_same_under_bulk(ix, Q, k, what)
        tsm.assert_answers(got, packed, HAND_DIM, metric, Q, k, None, what)
