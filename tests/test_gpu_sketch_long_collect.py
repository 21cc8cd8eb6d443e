"""The long-row collect form of the matrix sketch sweep and the long sample pass at 2 048 (32 steps, blocks of 256), 2 496
(39 steps: odd, the last with two column blocks) and 4 096 dimensions (the block of 512).  Without them the pass counts
(one per launch, not one per query) and sketch_topk_stats' queries fail."""
import numpy as np
import pytest

import test_gpu_sketch_long as tl
import test_gpu_sketch_matrix as tsm
import test_gpu_sketch_radius as tsr
import test_gpu_sketch_topk_collect as tc
from syzgydb_amd import _lib, cert_check as cc
from syzgydb_amd.index import sample_long_plan, scan_long_collect_plan

pytestmark = pytest.mark.gpu

EUC, COS = tsm.EUC, tsm.COS
# (dim, rows, queries of the call, sketch_wide) x metric
PARAMS = [(c, m) for c in [(2048, "s2", 16, 0), (2048, "2999", 19, 0), (2048, "s2", 32, 2), (2496, "2999", 16, 0),
                           (2496, "2999", 32, 2), (4096, "s2", 16, 0), (4096, "2999", 19, 0)] for m in (COS, EUC)]


def data(dim, rows):
    """test_gpu_sketch_long.data; where it has no 2 999-row corpus, the first 2 999 rows of its s2 corpus"""
    if rows == "s2" or dim in tl.SALT:
        return tl.data(dim, rows)
    packed, Q, _ = tl.data(dim, "s2")
    return packed[:int(rows)], Q, None


def loaded(ix, packed, seed):
    ix.load(packed) if seed is None else ix.synth(packed.shape[0], seed)


@pytest.mark.parametrize("case,metric", PARAMS, ids=["d%d-n%s-q%d-w%d-" % c + tsm.MID[m] for c, m in PARAMS])
def test_radius_hits_certificates_and_passes(case, metric):
    dim, rows, nq, wide = case
    packed, Qall, seed = data(dim, rows)
    n, Q = packed.shape[0], Qall[1:nq + 1]   # (query 0 coincides with a row: its m = 0 radius would be 0)
    corpus, what = cc.Corpus(packed, dim, 32, metric), ("long collect", case, tsm.MID[metric])
    dists = tsr.all_dists(corpus, Q)
    radii = tsr.radii_for(dists)
    sizes = [nq] if wide == 2 else tsm.launch_sizes(nq)   # (sketch_wide = 2: a call of up to 32 is ONE launch)
    plans = [scan_long_collect_plan(dim, 8, c, sketch_wide=wide) for c in sizes]
    assert all(p["serves"] and p["passes"] == 1 for p in plans), (what, plans)
    two = sizes[0] > 16
    assert plans[0]["blocks"] == (2 if two else 1) and plans[0]["block"] == (256 if dim <= 2496 and not two else 512), (what, plans)
    with tsr.open_radius(dim, metric, devices=[0], sketch_wide=wide) as ix:
        loaded(ix, packed, seed)
        got, st, _ = tsr.checked_call(ix, corpus, Q, radii, what, dists)
        tsr.assert_passes(st, n, dim, nq, len(plans), what)
        ix.set_option("sketch_matrix", 1)
        got1, st1, _ = tsr.checked_call(ix, corpus, Q, radii, what + ("sketch_matrix = 1",), dists)
        assert tsr.same_hits(got, got1), ("hits differ from the one-query collect kernel's", what)
        assert st["sketch_radius_fallbacks"] <= st1["sketch_radius_fallbacks"], (what, st, st1)
        tsr.assert_passes(st1, n, dim, nq, nq, what + ("sketch_matrix = 1",))


@pytest.mark.parametrize("dim", (2048, 4096))
def test_radius_overflow_is_regrown(dim):
    """Fresh buffers hold 1 024 entries per query: a query with 1 500 hits counts past collect_cap and is handed over; the
    regrown buffers settle it in the next call."""
    packed, Qall, seed = data(dim, "s2")
    n, Q, nq, corpus = packed.shape[0], Qall[1:17], 16, cc.Corpus(packed, dim, 32, COS)
    dists = tsr.all_dists(corpus, Q)
    radii = tsr.radii_for(dists, ms=(25,) * 5 + (1500,) + (25,) * 10)
    with tsr.open_radius(dim, COS, devices=[0]) as ix:
        loaded(ix, packed, seed)
        got, st, _ = tsr.checked_call(ix, corpus, Q, radii, ("overflow", dim), dists)
        _, st2, _ = tsr.checked_call(ix, corpus, Q, radii, ("regrown", dim), dists)
        assert len(got[5][0]) == 1500 and 1 <= st["sketch_radius_fallbacks"] > st2["sketch_radius_fallbacks"], (st, st2)
        tsr.assert_passes(st2, n, dim, nq, 2, ("regrown", dim))


@pytest.mark.parametrize("dim,metric", [(2048, COS), (2048, EUC), (4096, COS), (4096, EUC)])
def test_large_k_is_served_through_the_sketch(dim, metric):
    """k = 100, one call of 16: the long sample pass bounds the k-th distance (cert_check's S_k), the long collect sweep
    contains the answer."""
    k, nq = 100, 16
    packed, Qall, seed = data(dim, "s2")
    n, Q, corpus = packed.shape[0], Qall[1:nq + 1], cc.Corpus(packed, dim, 32, metric)
    sp = sample_long_plan(n, k, nq, dim)
    assert sp["serves"] and sp["blocks"] == 1 and sp["block"] == (256 if dim == 2048 else 512), sp
    dists = tc.all_dists(corpus, Q)
    with tc.open_tc(dim, metric, devices=[0]) as ix:
        loaded(ix, packed, seed)
        ix.reset_stats(), ix.certificates()
        got = ix.search_topk(Q, k)
        recs, ents, dropped = ix.certificates()
        st, ts, info = ix.stats(), ix.sketch_topk_stats(), ix.sketch_info()
        tc.assert_answers(got, tc.oracle_topk(corpus, Q, k, None), ("large k", dim))
        assert ts["queries"] + ts["fallbacks"] == nq and ts["queries"] >= nq - 1, ts
        cc.check(corpus, Q, recs, ents, dropped, dists=dists, what=("large k", dim),
                 sketch=(cc.Corpus(ix.sketch_rows()[0], dim, 8, metric), info["gscale"], info["exc_rows"]))
        # The sampled keys are the collect sweep's: kmax is the sampled key of rank k + its key_eps, an entry's ub its collected
        # key + its key_eps, so kmax is bit-equal to a collected sample row's ub and that row's key has rank k among theirs.
        in_sample = (np.arange(n) // 16) % sp["stride"] == 0
        assert not in_sample[np.asarray(info["exc_rows"], dtype=np.int64)].any(), ("an exception row in the sample", dim)
        own = recs[(recs["pass_"] == tc.PASS) & (recs["certified"] == 1)]
        assert len(own) == ts["queries"], (len(own), ts)
        for rec in own:
            e = ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]
            e = e[((e["flags"] & _lib.SZG_CERT_ENTRY_NO_KEY) == 0) & in_sample[e["row"].astype(np.int64)]]
            at = e["key"][e["ub"] == rec["kmax"]]
            assert at.size >= 1, ("kmax is no collected sample row's key plus its bound", dim, int(rec["query"]), float(rec["kmax"]))
            below, upto = int((e["key"] < at[0]).sum()), int((e["key"] <= at[0]).sum())
            assert below < k <= upto, ("the sampled key's rank among the collected keys is not k", dim, int(rec["query"]), below, upto)
        if tsm.DEFAULT_TUNABLES and ts["fallbacks"] == 0:   # one sample launch of 16, collect launches of 12 and 4
            sample_rows = (sp["tiles"] - 1) * 16 + min(16, n - (sp["tiles"] - 1) * sp["stride"] * 16)
            assert st["scan_bytes"] == (sample_rows + 2 * n) * dim, (st, sp)


@pytest.mark.parametrize("metric", (COS, EUC), ids=["cos", "euc"])
def test_every_key_at_4096_against_the_wide_reference(metric):
    """3 queries x 1 605 rows within cert_check.WIDE_LIMIT: the collected keys against the extended-precision reference."""
    dim, n = 4096, 1605
    packed, Qall, _ = data(dim, "s2")
    corpus, Q = cc.Corpus(packed[:n], dim, 32, metric), Qall[1:4]
    assert 3 * n * dim <= cc.WIDE_LIMIT and scan_long_collect_plan(dim, 8, 3)["serves"]
    dists = tsr.all_dists(corpus, Q)
    radii = tsr.radii_for(dists, ms=(300, 25, 1))
    with tsr.open_radius(dim, metric, devices=[0]) as ix:
        ix.load(packed[:n])
        _, st, recs_all = tsr.checked_call(ix, corpus, Q, radii, ("long collect, wide reference", tsm.MID[metric]), dists)
        assert sum(int(r["n_entries"]) for r in recs_all[0][0]) >= 300 * (st["sketch_radius_fallbacks"] == 0)
        tsr.assert_passes(st, n, dim, 3, 1, "4096 wide reference")
