"""The matrix sketch sweep's long-row form (kernels_scan_mx.hip -DSZG_MX_LONG) at 1 920, 2 048 and 4 096 dimensions.
1 920 is the first dimension the form takes (30 steps: no multiple of its ring of 8); at 1 024 .. 1 856 the plan keeps the
one-block form of 64 KiB, which measured faster: the issue's 1 024 has no long launch to test.  Under
sketch_wide = 2 and sketch_share = 2 a call of 19 or 32 queries is ONE wide launch, of 37 or 64 ONE shared launch; 16 are
two launches (12 and 4).  Lists of 12: row lists, and the serial inserts under sketch_select = 1.

Row counts.  A sweep spreads its tiles of 16 rows over 2 048 waves.  The one-block and wide launches run on "s2" = two
steps of the launch plus 77 rows (65 613): every wave walks two tiles and the first five three -- the accumulators'
reset, the next tile's first A operands, the ring across a tile's end, lists that fill and reject.  The shared launches
pair their blocks: 96 waves for the 188 tiles of 2 999 uniform rows (a ragged last tile); a wide launch of 19 runs there too.

Checked: every list key within key_eps of its float64 key (cert_check), ids and distances == the oracle's, no more queries
handed over than under sketch_matrix = 1 (none but one of 16 at 4 096 Euclidean, in both), and the passes of
szg_stats.scan_bytes against szg_debug_scan_long's -- exact where every query settled, modulo 4 otherwise (a query handed
over adds 4; the grouped kernels' count differs by 2) -- which is how the test knows the long kernels ran.
"""
import functools

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import scan_long_plan
import test_gpu_sketch_matrix as tsm

pytestmark = pytest.mark.gpu

K = 10
EUC, COS = tsm.EUC, tsm.COS
# (dim, rows, queries of the call, sketch_select): lists of 12 entries -- row lists, or under sketch_select = 1 the serial
# inserts (lists of more than 16 entries, which take them unasked, do not fit the one-launch merge of 512 block lists)
CASES = sorted([(1920, "s2", 16, 0), (1920, "s2", 32, 0), (2048, "s2", 16, 0), (2048, "s2", 16, 1), (2048, "s2", 32, 0),
                (4096, "s2", 16, 0), (4096, "s2", 16, 1)] +
               [(dim, "2999", nq, 0) for dim in (1920, 2048) for nq in (19, 37, 64)])   # (one corpus at a time)
LIST = 12
PARAMS = [(c, m) for c in CASES for m in (COS, EUC)]
# Seeds of the 2 999-row corpora, checked on the CPU: a shared launch leaves 12 lists per query, and of a query's 60 best
# rows at most 12 fall into one of them under both metrics: lists of 12 drop none, no query is handed over for their sake
SALT = {1920: 4, 2048: 2}


@functools.lru_cache(maxsize=1)
def data(dim, rows):
    """-> (packed float32 rows, 64 queries, the seed of ix.synth or None); query 0 coincides with stored row 211"""
    if rows == "s2":
        n, seed = 2 * tsm.rows_per_step(dim) + 77, 0x4C4F4E47 + dim
        packed, Q = tsm.synth_corpus(seed, n, dim), orc.synth_vectors(seed + 1, 0, 64, dim) * 0.7
    else:
        rng = np.random.default_rng(0x4C4F4E47 + dim + SALT[dim])
        V = rng.uniform(-1, 1, (int(rows), dim)).astype(np.float32).astype(np.float64)
        packed, Q, seed = orc.encode_rows(V, 32), rng.uniform(-1, 1, (64, dim)), None
    Q[0] = orc.decode_vector(packed[211], dim, 32)
    return packed, Q, seed


def certified_call(ix, corpus, Q, what, dists=None):
    """One call: the sketch records' keys and bounds against float64 (cc.check), the answers against the oracle."""
    ix.reset_stats()
    got = ix.search_topk(Q, K)
    st = ix.stats()
    recs, ents, dropped = ix.certificates()
    info = ix.sketch_info()
    sk_corpus = cc.Corpus(ix.sketch_rows()[0], corpus.dim, 8, corpus.metric)
    if dists is None:
        dists = np.stack(list(tsm.POOL.map(lambda q: orc.all_distances(corpus.packed, corpus.dim, 32, corpus.metric, q), Q)))
    s = cc.check(corpus, Q, recs, ents, dropped, dists=dists, margins=tsm.MARGINS, what=what,
                 sketch=(sk_corpus, info["gscale"], info["exc_rows"]))
    assert s.skipped == 0 and s.checked > 0, (what, s.skipped, s.checked)
    tsm.assert_answers(got, corpus.packed, corpus.dim, corpus.metric, Q, K, None, what)
    return got, st, s.checked, dists


@pytest.mark.parametrize("case,metric", PARAMS, ids=["d%d-n%s-q%d-s%d-" % c + tsm.MID[m] for c, m in PARAMS])
def test_answers_keys_and_passes(case, metric):
    dim, rows, nq, select = case
    packed, Qall, seed = data(dim, rows)
    n, Q = packed.shape[0], Qall[:nq]
    corpus = cc.Corpus(packed, dim, 32, metric)
    plans = [scan_long_plan(dim, 8, c, kp=LIST) for c in ([nq] if nq > 16 else tsm.launch_sizes(nq))]
    what = ("long rows", case, tsm.MID[metric])
    assert all(p["serves"] for p in plans), (what, plans)
    assert plans[0]["blocks"] == (2 if nq > 16 else 1) and plans[0]["share"] == (nq > 32), (what, plans)
    want = sum(p["passes"] for p in plans)
    assert want == (1 if nq <= 32 else 2) * len(plans), (what, plans)
    with tsm.open_sketched(dim, metric, devices=[0], sketch_wide=2, sketch_share=2, sketch_list=LIST, sketch_select=select) as ix:
        if seed is None:
            ix.load(packed)
        else:
            ix.synth(n, seed)
        _, st, checked, dists = certified_call(ix, corpus, Q, what)
        print(what, "rows", n, "keys checked", checked, "settled", st["sketch_queries"], "passes", tsm.sketch_passes(st, n, dim, what))
        tsm.assert_pass_count(st, n, dim, nq, want, what)
        ix.set_option("sketch_matrix", 1)
        _, st1, _, _ = certified_call(ix, corpus, Q, what + ("sketch_matrix = 1",), dists=dists)
        assert st["sketch_queries"] >= st1["sketch_queries"] and st["sketch_fallbacks"] <= st1["sketch_fallbacks"], (what, st, st1)
        if tsm.DEFAULT_TUNABLES and st1["sketch_queries"] == nq:
            assert tsm.sketch_passes(st1, n, dim, what) > want, ("the grouped kernels make more passes", what, st1)


@pytest.mark.parametrize("metric", (COS, EUC), ids=["cos", "euc"])
def test_every_key_at_4096_against_the_wide_reference(metric):
    """3 queries x 1 605 rows x 4 096 dimensions stay within cert_check.WIDE_LIMIT: the float64 keys come from the
    element-by-element extended-precision reference, which resolves the key of the query that coincides with row 211.
    Lists of 24 entries (serial inserts) beside the 128 KiB image.  (One tile per wave: the s2 cases walk several.)"""
    dim, n = 4096, 1605
    packed, Qall, _ = data(dim, "s2")
    corpus = cc.Corpus(packed[:n], dim, 32, metric)
    assert 3 * n * dim <= cc.WIDE_LIMIT and scan_long_plan(dim, 8, 3, kp=24)["serves"]
    with tsm.open_sketched(dim, metric, devices=[0], sketch_list=24) as ix:
        ix.load(packed[:n])
        got, st, checked, _ = certified_call(ix, corpus, Qall[:3], ("long rows, wide reference", tsm.MID[metric]))
        # (cosine: the reference's unclamped acos may give NaN at a parallel pair, which sorts last -- the oracle decides)
        assert checked >= 3 * K and (metric == COS or int(got[0][0, 0]) == 211), (checked, got[0][0])
        tsm.assert_pass_count(st, n, dim, 3, 1, "4096 wide reference")
