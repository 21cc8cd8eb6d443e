"""The matrix sketch sweep's shared form (kernels_scan_mx.hip built with SZG_MX_SHARE; option sketch_share): ONE launch of
33 to 64 queries as two column groups of 32.  The grid has 2 S blocks; share_map gives a block its row slice and its
group, the two blocks of a slice walk the same tiles, and each query gets S block lists.

sketch_share = 2 forces it: every sketch call of more than 32 queries goes in batches of up to 64 from its first query
on.  Per case the same call runs under sketch_share 2 and 1 and is compared: the answers (ids, distances, counts) byte
for byte, and every entry that both traces hold for a query key bit for key bit.  The lists of a shared launch are
short (row lists hold at most 16 entries, a call keeps 47 or more candidates), and S differs from the plain grid: which
rows a query's merged list holds, and its drop bound, legitimately depend on the partition and are not compared; where
the form does not serve (the controls: one block of rows under sketch_list = 0 keeps full lists) both settings take the
same launches and records and entries are equal byte for byte.  Under 2: the certificate chain (K_s, L_s, D, S) and the
oracle's answers as in test_gpu_sketch_matrix.py; szg_stats.scan_launches and the pass count of scan_bytes, which is how
a test knows the shared kernel ran -- one launch and two passes per batch of 33 to 64; and the call three times over with
identical traces: which partner of a slice runs ahead changes nothing.

Shapes: the any-steps kernel (64), the 6-step (384) and the 12-step one (768).  Rows: 15, 16, 17 (one tile: S = 1, three
waves of each block without a tile), 192 (a plain grid of 3: an odd grid, S = 1), 20 000 (a plain grid of 313, S = 156:
neither grid a multiple of 16 -- share_map's fallback -- and 1 250 tiles, no multiple of S x 4 waves), and one / three steps
of the launch plus 77 (grid 512, S = 256, partners b and b + 8).  Queries: 33 (one live column in the second group), 48,
63, 64, 65 (a shared launch and a lone query), 96 (shared, then a wide launch of 32) and 97 (two shared launches).
"""
import pytest

import oracle as orc
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import scan_plan, scan_share_plan, merge_short_plan
import test_gpu_sketch_matrix as tsm
import test_gpu_sketch_select as tss
import test_gpu_sketch_wide as tsw

pytestmark = pytest.mark.gpu

SEED = 0x53595A470000F000
EUC, COS = tsm.EUC, tsm.COS
MID = tsm.MID


def share_geom(dim, n, k, want):
    """(S, m) of a shared launch (scan_topk.cpp, share_geometry): grid 2 S, S = max(1, plain grid / 2)."""
    kp = tsm.sketch_kp(k)
    S = max(1, scan_plan(dim, 8, n, kp=kp)["grid"] // 2)
    m = want if want > 0 else max(8, 2 * kp // S + 8)
    return S, (kp if m >= kp or not merge_short_plan(S, m, kp)["fits"] else m)


def share_serves(dim, n, k, want):
    """sketch_share_serves: the wide form serves the plain launch, and scan_variant names the shared form at S lists."""
    return tsw.wide_serves(dim, n, k, want) and scan_share_plan(dim, 8, 64, kp=share_geom(dim, n, k, want)[1], sketch_share=2)["serves"]


def forced_batches(nq):
    """Batches of a call under sketch_share = 2: up to 64 queries each, from the first query on."""
    return [64] * (nq // 64) + ([nq % 64] if nq % 64 else [])


def forced_passes(nq):
    return sum(2 if b > 32 else 1 for b in forced_batches(nq))


def test_plans_of_this_file():
    assert [forced_batches(q) for q in (33, 64, 65, 96, 97)] == [[33], [64], [64, 1], [64, 32], [64, 33]]
    assert [forced_passes(q) for q in (33, 48, 63, 64, 65, 96, 97)] == [2, 2, 2, 2, 3, 3, 4]
    for nq in (33, 48, 63, 64, 65, 96, 97):   # the hook splits the call the same way
        p = scan_share_plan(768, 8, nq, sketch_share=2)
        assert (p["batches"], p["launches"], p["passes"]) == (forced_batches(nq), len(forced_batches(nq)), forced_passes(nq)), (nq, p)
    for dim in (64, 384, 768):
        assert share_serves(dim, 17, 10, 8) and not share_serves(dim, 17, 10, 0)
        assert share_serves(dim, 192, 10, 8) and not share_serves(dim, 192, 10, 0)
        for rows in (20000, "s1", "s3"):
            assert share_serves(dim, tsm.n_rows_of(dim, rows), 10, 0) and share_serves(dim, tsm.n_rows_of(dim, rows), 1, 8)
        assert share_geom(dim, 17, 10, 8)[0] == 1 and share_geom(dim, 192, 10, 8)[0] == 1
        assert share_geom(dim, 20000, 10, 8)[0] == 156 and share_geom(dim, tsm.n_rows_of(dim, "s1"), 10, 8)[0] == 256
    assert scan_plan(768, 8, 192, kp=60)["grid"] == 3 and scan_plan(768, 8, 20000, kp=60)["grid"] == 313
    assert (20000 + 15) // 16 % (156 * 4) != 0


def traced_keys(t, q):
    """row -> the key's bits, of the entries of query q's sketch record that carry a key (the list entries)"""
    e = t[q][3]
    keyed = e[(e["flags"] & tss._lib.SZG_CERT_ENTRY_NO_KEY) == 0] if "flags" in e.dtype.names else e
    return {int(r): k.tobytes() for r, k in zip(keyed["row"], keyed["key"])}


def assert_same_under_share(ix, Q, k, what, full_lists):
    """The call under sketch_share 2 (three times) and 1.  -> the answers under 2"""
    seen = {}
    ix.set_option("sketch_share", 2)
    runs = [tss.traced_call(ix, Q, k, what + ("sketch_share", 2, "run", i)) for i in range(3)]
    ix.set_option("sketch_share", 1)
    seen[1] = tss.traced_call(ix, Q, k, what + ("sketch_share", 1))
    ix.set_option("sketch_share", 2)
    g2, b2, t2 = runs[0]
    for i in (1, 2):   # drift between the partners of a slice changes nothing
        gi, bi, ti = runs[i]
        assert bi == b2, ("scan_bytes differ between runs", what, i)
        for a, b in zip(gi, g2):
            assert a.tobytes() == b.tobytes(), ("answers differ between runs", what, i)
        for q in range(Q.shape[0]):
            assert ti[q][0] == t2[q][0] and ti[q][1] == t2[q][1], ("traces differ between runs", what, i, q)
    g1, b1, t1 = seen[1]
    for a, b in zip(g2, g1):
        assert a.tobytes() == b.tobytes(), ("answers differ from sketch_share = 1", what)
    common = 0
    for q in range(Q.shape[0]):
        k2, k1 = traced_keys(t2, q), traced_keys(t1, q)
        both = set(k2) & set(k1)
        common += len(both)
        for r in both:
            assert k2[r] == k1[r], ("key bits differ", what, q, r)
        if full_lists:
            assert t2[q][1] == t1[q][1], ("entries differ", what, q)
            assert t2[q][0] == t1[q][0], ("records differ", what, q)
    assert common >= Q.shape[0], ("the two traces share no entries", what, common)
    return g2


# ---- the lattice ---------------------------------------------------------------------------------------------------
DIMS = (64, 384, 768)
SMALL = (15, 16, 17, 192)
ROWS = SMALL + (20000, "s1", "s3")
NQS = (33, 48, 63, 64, 65, 96, 97)
KS = (1, 10)
LISTS = (0, 8)


def lattice():
    """Per kernel form every row count, query count, metric, k and sketch_list; the offsets differ from form to form.
    One block of rows keeps its full lists under sketch_list = 0 (the control, one per form): the small row counts take
    lists of 8 elsewhere, so that every query count runs the shared kernel in every form."""
    out = []
    for d, dim in enumerate(DIMS):
        for i, rows in enumerate(ROWS):
            lst = 8 if rows in SMALL else LISTS[(i + d) % 2]
            out.append((dim, rows, NQS[(i + 2 * d) % 7], (i + d) % 2, KS[(i + d // 2) % 2], lst))
        out.append((dim, SMALL[d], 33, d % 2, 10, 0))   # the control
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
        served = [c for c in mine if share_serves(dim, tsm.n_rows_of(dim, c[1]), c[4], c[5])]
        assert {c[2] for c in served} == set(NQS), (dim, "every query count runs the shared kernel")
        assert {c[1] for c in served} == set(ROWS), (dim, "every row count runs the shared kernel")
        assert len(served) == len(mine) - 1, dim


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_same_answers_and_keys_shared_and_not(case):
    dim, rows, nq, metric, k, lst = case
    n = tsm.n_rows_of(dim, rows)
    seed = SEED + dim * 100 + (n % 1000) + k
    corpus = cc.Corpus(tsm.synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    what = ("share", case_id(case), "rows", n)
    served = share_serves(dim, n, k, lst)
    with tsm.open_sketched(dim, metric, sketch_list=lst, sketch_share=2) as ix:
        ix.synth(n, seed)
        assert_same_under_share(ix, Q, k, what, full_lists=not served)
        got, st, checked, settled, _ = tsm.certified_call(ix, corpus, Q, k, what)
        assert st["sketch_queries"] + st["sketch_fallbacks"] == nq and st["mq_queries"] == 0, (what, st)
        print(what, "shared kernel", served, "launches", st["scan_launches"], "keys checked", checked, "settled", settled)
        if served:
            tsm.assert_pass_count(st, n, dim, nq, forced_passes(nq), what)
            if tsm.DEFAULT_TUNABLES:
                assert st["scan_launches"] >= len(forced_batches(nq)), (what, st)
                if st["sketch_queries"] == nq and st["escalations"] == 0 and st["full_replays"] == 0:
                    assert st["scan_launches"] == len(forced_batches(nq)), (what, st)
        elif nq < 72:   # (the call keeps the default plan)
            tsm.assert_pass_count(st, n, dim, nq, tsm.matrix_passes(nq), what)


# ---- the automatic rule ------------------------------------------------------------------------------------------------
AUTO_DIM, AUTO_ROWS = tsw.AUTO_DIM, tsw.AUTO_ROWS


def launches_of(ix, Q, k, n, dim, what):
    ix.reset_stats()
    got = ix.search_topk(Q, k)
    st = ix.stats()
    return got, st, tsm.sketch_passes(st, n, dim, what)


@pytest.mark.parametrize("nq,batches", ((135, [4, 32, 32, 32, 31, 4]), (136, [4, 64, 64, 4])))
def test_automatic_rule(nq, batches):
    dim, n, k = AUTO_DIM, AUTO_ROWS, 10
    seed = SEED + 77
    packed = tsm.synth_corpus(seed, n, dim)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    assert share_serves(dim, n, k, 0)
    assert scan_share_plan(dim, 8, nq)["batches"] == batches
    with tsm.open_sketched(dim, COS) as ix:
        ix.synth(n, seed)
        ix.set_option("sketch_share", 1)
        got1, st1, p1 = launches_of(ix, Q, k, n, dim, "sketch_share = 1")
        ix.set_option("sketch_share", 0)
        for ft in (1, 0):
            ix.set_option("finish_thread", ft)
            got, st, p = launches_of(ix, Q, k, n, dim, ("automatic", "finish_thread", ft))
            assert tsm.same(got, got1), ("answers differ from sketch_share = 1", nq, ft)
            assert st["sketch_queries"] + st["sketch_fallbacks"] == nq, st
            print("automatic", nq, "finish_thread", ft, "launches", st["scan_launches"], "passes", p, "settled", st["sketch_queries"])
            if tsm.DEFAULT_TUNABLES and st["sketch_queries"] == nq and st["escalations"] == 0 and st["full_replays"] == 0:
                assert st["scan_launches"] == len(batches), (nq, ft, st)
                assert p == sum(2 if b > 32 else 1 for b in batches), (nq, ft, p)
                assert st1["scan_launches"] == len(tsw.auto_batches(nq)) and p1 == len(tsw.auto_batches(nq)), (nq, st1, p1)
        ix.set_option("finish_thread", 1)
        tsm.assert_answers(got, packed, dim, COS, Q, k, None, ("automatic", nq))
