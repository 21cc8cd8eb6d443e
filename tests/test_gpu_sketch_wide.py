"""The matrix sketch sweep's two-block form (kernels_scan_mx.hip, NB = 2; option sketch_wide): a launch of 17 to 32 queries
with row lists scores two column blocks of 16 queries per row read -- slot 4 b + r of lane-row c is the list of query
16 b + 4 c + r.

sketch_wide = 2 forces it: every sketch call of more than 16 queries goes in batches of up to 32, one launch each.  Per
case the same call runs under sketch_wide 2 and 1 (the 16-query launches) and everything the sweep hands on is compared
byte for byte -- the certificate trace's sketch records (lb carries the drop bound) with their entries (rows, keys,
bounds, distances) and the answers.  Under 2 alone: the certificate chain (K_s, L_s, D, S) and the oracle's answers as in
test_gpu_sketch_matrix.py, and the pass count of szg_stats.scan_bytes, which is how a test knows the wide kernel ran:
one pass per launch of up to 32.

Shapes: the any-steps kernel (64), the 6-step (384) and the 12-step one (768); rows below, at and above one tile, and
one / three steps of the launch plus 77; 17 queries (one live column in the second block), 31, 32, 33 (a wide launch
and a lone query) and 48 (a wide launch and a one-block launch of 16).  Lists: the row-list form needs lists of at most
16 entries -- up to 64 rows lie in ONE block, whose automatic list is the call's whole kp: such cases (sketch_list = 0 on
15 to 17 rows) are the control, the one-block serial inserts under both settings.
"""
import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import scan_plan, scan_wide_plan, merge_short_plan
import test_gpu_sketch_matrix as tsm
import test_gpu_sketch_select as tss

pytestmark = pytest.mark.gpu

SEED = 0x53595A470000D000
EUC, COS = tsm.EUC, tsm.COS
MID = tsm.MID


def list_len(dim, n, k, want):
    """Entries per wave and block list of the call's sweeps (scan_topk.cpp, sketch_list_len)."""
    kp = tsm.sketch_kp(k)
    grid = scan_plan(dim, 8, n, kp=kp)["grid"]
    m = want if want > 0 else max(8, 2 * kp // grid + 8)
    return kp if m >= kp or not merge_short_plan(grid, m, kp)["fits"] else m


def wide_serves(dim, n, k, want):
    m = list_len(dim, n, k, want)
    return scan_wide_plan(dim, 8, 32, kp=m, sketch_wide=2)["serves"]


def forced_batches(nq):
    """Batches of a call under sketch_wide = 2: up to 32 queries each, from the first query on."""
    return [32] * (nq // 32) + ([nq % 32] if nq % 32 else [])


def forced_passes(nq):
    return sum(1 if b > 16 else -(-b // 16) for b in forced_batches(nq))


def auto_batches(nq):
    """Batches of a call of 72 queries or more under sketch_wide = 0: 4, 32 ..., a rest, 4 (plan_batch)."""
    assert nq >= 72
    out, q0 = [], 0
    while q0 < nq:
        left = nq - q0
        n = min(32, left)
        if left > 4:
            n = min(n, 4) if q0 == 0 else (left - 4 if left <= 36 else n)
        out.append(n)
        q0 += n
    return out


def test_plans_of_this_file():
    assert [forced_passes(q) for q in (17, 31, 32, 33, 48)] == [1, 1, 1, 2, 2]
    assert auto_batches(72) == [4, 32, 32, 4] and auto_batches(100) == [4, 32, 32, 28, 4]
    assert auto_batches(80) == [4, 32, 32, 8, 4]
    for dim in (64, 384, 768):   # lists of 8 on any row count; one block of rows keeps the whole kp
        assert wide_serves(dim, 17, 10, 8) and not wide_serves(dim, 17, 10, 0)
        assert wide_serves(dim, tsm.n_rows_of(dim, "s1"), 10, 0)


def assert_same_under_wide(ix, Q, k, what):
    """The call under sketch_wide 2 and 1: records, drop bound, entries and answers byte for byte.
    -> (answers, scan_bytes under 2, scan_bytes under 1)"""
    seen = {}
    for w in (2, 1):
        ix.set_option("sketch_wide", w)
        seen[w] = tss.traced_call(ix, Q, k, what + ("sketch_wide", w))
    ix.set_option("sketch_wide", 2)
    (g2, b2, t2), (g1, b1, t1) = seen[2], seen[1]
    for q in range(Q.shape[0]):
        r2, r1 = t2[q][2], t1[q][2]
        assert r2["thr_min"].tobytes() == r1["thr_min"].tobytes(), ("drop bound / lb differs", what, q, r2["thr_min"], r1["thr_min"])
        assert int(r2["n_entries"]) == int(r1["n_entries"]), ("entry counts differ", what, q)
        e2, e1 = t2[q][3], t1[q][3]
        assert (e2["row"] == e1["row"]).all(), ("rows differ", what, q, e2["row"], e1["row"])
        assert e2["key"].tobytes() == e1["key"].tobytes(), ("keys differ", what, q)
        assert t2[q][1] == t1[q][1], ("entries differ", what, q)
        assert t2[q][0] == t1[q][0], ("records differ", what, q, r2, r1)
    for a, b in zip(g2, g1):
        assert a.tobytes() == b.tobytes(), ("answers differ", what)
    return g2, b2, b1


# ---- the lattice ---------------------------------------------------------------------------------------------------
DIMS = (64, 384, 768)
ROWS = (15, 16, 17, "s1", "s3")
NQS = (17, 31, 32, 33, 48)
KS = (1, 10)
LISTS = (0, 8)


def lattice():
    """Per kernel form every row count, query count, metric, k and sketch_list; the offsets differ from form to form."""
    out = []
    for d, dim in enumerate(DIMS):
        for i, rows in enumerate(ROWS):
            out.append((dim, rows, NQS[(i + 2 * d) % 5], (i + d) % 2, KS[(i + d) % 2], LISTS[(i + (d + 1) // 2) % 2]))
        # lists of 8 on one tile (one block, one live column in the second column block) and on three steps
        out.append((dim, 16, 17, (d + 1) % 2, 10, 8))
        # (the query count whose case above is a control: every count runs the wide kernel in every form)
        out.append((dim, "s3", (32, 33, 48)[d], d % 2, 10, 8))
    return out


CASES = lattice()


def case_id(c):
    dim, rows, nq, metric, k, lst = c
    return "d%d-n%s-q%d-%s-k%d-l%d" % (dim, rows, nq, MID[metric], k, lst)


def test_lattice_covers_every_value_with_every_form():
    for dim in DIMS:
        mine = [c for c in CASES if c[0] == dim]
        assert {c[1] for c in mine} == set(ROWS) and {c[2] for c in mine} == set(NQS), dim
        assert {c[3] for c in mine} == {EUC, COS} and {c[4] for c in mine} == set(KS) and {c[5] for c in mine} == set(LISTS), dim
        wide = [c for c in mine if wide_serves(dim, tsm.n_rows_of(dim, c[1]), c[4], c[5])]
        assert {c[2] for c in wide} == set(NQS), (dim, "every query count runs the wide kernel")
        assert {c[1] for c in wide} >= {16, "s1", "s3"}, dim


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_same_lists_wide_and_narrow(case):
    dim, rows, nq, metric, k, lst = case
    n = tsm.n_rows_of(dim, rows)
    seed = SEED + dim * 100 + (n % 1000) + k
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    what = ("wide", case_id(case), "rows", n)
    wide = wide_serves(dim, n, k, lst)
    with tsm.open_sketched(dim, metric, sketch_list=lst, sketch_wide=2) as ix:
        ix.synth(n, seed)
        assert_same_under_wide(ix, Q, k, what)
        got, st, checked, settled, _ = tsm.certified_call(ix, corpus, Q, k, what)
        assert st["sketch_queries"] + st["sketch_fallbacks"] == nq and st["mq_queries"] == 0, (what, st)
        # (where the two-block form does not serve the call's launches, the call keeps the default plan)
        want = forced_passes(nq) if wide else tsm.matrix_passes(nq)
        tsm.assert_pass_count(st, n, dim, nq, want, what)
        print(what, "wide kernel", wide, "keys checked", checked, "settled", settled)


# ---- equal keys in the second block's slots --------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 2, 8, 16))
@pytest.mark.parametrize("nq", (32, 21))
def test_improving_pairs_in_the_second_block(m, nq):
    """test_gpu_sketch_select.py's improving pairs -- every ladder row twice, better rows after them -- aimed at the
    queries of the second column block (16 ..), the first block's queries looking the other way: 16 passing lanes per
    lane-row and tile in slots 4 .. 7, equal keys side by side, and which of two leaves a full list is decided by the
    row half of the 64-bit compare alone."""
    n, k, dim = 47, 10, tss.HAND_DIM
    rng = np.random.default_rng(6200 + n)
    V, q = tss.ladder((n + 1) // 2, rng)
    V = np.repeat(V, 2, axis=0)[:n].astype(np.float32).astype(np.float64)
    jitter = 1e-3 * rng.standard_normal((nq, dim))
    Q = np.stack([(q if x >= 16 else -q) + jitter[x] for x in range(nq)])
    packed = orc.encode_rows(V, 32)
    assert scan_wide_plan(dim, 8, nq, kp=m, sketch_wide=2)["serves"]
    for metric in (COS, EUC):
        what = ("improving pairs, second block", "m", m, "queries", nq, MID[metric])
        dists = np.stack([orc.all_distances(packed, dim, 32, metric, x) for x in Q])
        for x in range(16, nq):
            step = np.diff(dists[x])
            assert (step[0::2] == 0).all() and (step[1::2] < 0).all(), (what, x)
        with tsm.open_sketched(dim, metric, sketch_list=m, sketch_wide=2) as ix:
            ix.load(packed)
            got, b2, b1 = assert_same_under_wide(ix, Q, k, what)
            tsm.assert_answers(got, packed, dim, metric, Q, k, None, what)


# ---- the automatic rule, the finisher thread, queries handed over -----------------------------------------------------
AUTO_DIM, AUTO_ROWS = 64, 3000


def passes_of(ix, Q, k, n, dim, what):
    ix.reset_stats()
    got = ix.search_topk(Q, k)
    st = ix.stats()
    return got, st, tsm.sketch_passes(st, n, dim, what)


def test_automatic_rule_and_finisher_thread():
    dim, n, k = AUTO_DIM, AUTO_ROWS, 10
    seed = SEED + 77
    packed = tsm.synth_corpus(seed, n, dim)
    Q = orc.synth_vectors(seed + 1, 0, 100, dim) * 0.7
    assert wide_serves(dim, n, k, 0)
    with tsm.open_sketched(dim, COS) as ix:
        ix.synth(n, seed)
        ix.set_option("sketch_wide", 1)
        got1, st1, p1 = passes_of(ix, Q, k, n, dim, "sketch_wide = 1")
        got1_40, _, p1_40 = passes_of(ix, Q[:40], k, n, dim, "sketch_wide = 1, 40 queries")
        ix.set_option("sketch_wide", 0)
        runs = {}
        for ft in (1, 0):
            ix.set_option("finish_thread", ft)
            runs[ft] = passes_of(ix, Q, k, n, dim, ("automatic", "finish_thread", ft))
        ix.set_option("finish_thread", 1)
        for ft in (1, 0):
            got, st, p = runs[ft]
            assert tsm.same(got, got1), ("answers differ from sketch_wide = 1", ft)
            assert st["sketch_queries"] + st["sketch_fallbacks"] == 100, st
            if tsm.DEFAULT_TUNABLES and st["sketch_queries"] == 100:
                assert p == len(auto_batches(100)) == 5, (ft, p)   # one pass per batch: 4, 32, 32, 28, 4
                assert p1 == tsm.matrix_passes(100), p1
        # a call below the threshold keeps its plan: [4, 16, 16, 4]
        got40, st40, p40 = passes_of(ix, Q[:40], k, n, dim, "automatic, 40 queries")
        assert tsm.same(got40, got1_40)
        if tsm.DEFAULT_TUNABLES and st40["sketch_queries"] == 40:
            assert p40 == p1_40 == tsm.matrix_passes(40) == 4, (p40, p1_40)
        tsm.assert_answers(runs[1][0], packed, dim, COS, Q, k, None, "automatic, 100 queries")


def test_every_query_handed_over_comes_back_in_order():
    """Every row twice under tie_mode = 0: two equal distances among each query's best k + 1, so the sketch settles
    none and the full sweep answers all 100 -- each in its own place."""
    dim, n, k = AUTO_DIM, AUTO_ROWS, 10
    seed = SEED + 78
    half = tsm.synth_corpus(seed, n // 2, dim)
    packed = np.repeat(half, 2, axis=0)
    Q = orc.synth_vectors(seed + 1, 0, 100, dim) * 0.7
    for ft in (1, 0):
        with tsm.open_sketched(dim, COS, tie_mode=0, finish_thread=ft) as ix:
            ix.load(packed)
            ix.reset_stats()
            got = ix.search_topk(Q, k)
            st = ix.stats()
            assert st["sketch_fallbacks"] == 100 and st["sketch_queries"] == 0, (ft, st)
            tsm.assert_answers(got, packed, dim, COS, Q, k, None, ("all handed over", "finish_thread", ft))
