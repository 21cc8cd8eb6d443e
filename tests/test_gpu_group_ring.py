"""Ring depth of the grouped 8-bit sweeps (option "scan_group_ring"): the G > 1 row-shape kernels exist at
more than one depth of the piece ring.  The depth only decides how far ahead a lane loads, so keys, lists, certificates
and answers are bit for bit those of every other depth and of scan_group = 1.

Row counts are built from the launch's own geometry (scan_plan): with S rows per step of the whole launch, n = s S + r
gives every wave s row steps (one more for the first r rows' waves).  s = 1 never enters the dense ring, s = 2 is its
shortest run, s = 3 is one trip of the whole-row loop plus the guarded drain at every compiled depth (12 pieces per row,
depths up to 12: the loop needs consumed + D + 12 <= 36), s = 5 several trips; r = 1 and 77 leave a ragged last step.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import ScanIndex, SZG_COSINE, SZG_EUCLIDEAN, _lib, cert_check as cc
from syzgydb_amd.index import scan_plan, scan_group_plan, scan_group_ring_plan, option_check

pytestmark = pytest.mark.gpu

SEED = 0x53595A4700005000
DEFAULT_TUNABLES = not os.environ.get("SZG_OPTIONS")   # (an option sweep may change the call plan, never the answers)
POOL = ThreadPoolExecutor(8)     # the oracle's C calls release the interpreter lock
DIMS = (768, 384, 100)           # the two row-shape kernels and an any-shape lane map
STEPS = (1, 2, 3, 5)
RAGGED = (0, 1, 77)
N_QUERIES = (3, 16, 17)          # an idle slot in the last group, a full launch, a launch plus one
K = 10
KP_PLAIN = 26                    # k + slack of a plain handle at k = 10
CASES = [(dim, s, r, m) for dim in DIMS for s in STEPS for r in RAGGED for m in (SZG_EUCLIDEAN, SZG_COSINE)]
IDS = ["%d-s%d-r%d-%s" % (dim, s, r, "cos" if m == SZG_COSINE else "euc") for dim, s, r, m in CASES]


def rows_per_step(dim):
    p = scan_plan(dim, 8, 1 << 22, kp=KP_PLAIN)
    return p["grid"] * (p["block"] // 64) * 16 if p["tiled"] else p["grid"] * (p["block"] // 64) * p["gpw"]


def depths(dim):
    """the values of scan_group_ring to compare: automatic and every depth the library carries"""
    return [0] + scan_group_ring_plan(dim, 8, 16, kp=KP_PLAIN, scan_group=4)["depths"]


@functools.lru_cache(maxsize=1)
def packed(seed, n, dim, bits):
    cuts = np.linspace(0, n, 9).astype(np.int64)
    parts = POOL.map(lambda i: orc.synth_rows(seed, int(cuts[i]), int(cuts[i + 1] - cuts[i]), dim, bits), range(8))
    return np.concatenate(list(parts))


def same(a, b):
    (ra, da, ca), (rb, db, cb) = a, b
    if not (ca == cb).all():
        return False
    for qi in range(len(ca)):
        n = ca[qi]
        if not (ra[qi, :n] == rb[qi, :n]).all() or not (da[qi, :n].view(np.uint64) == db[qi, :n].view(np.uint64)).all():
            return False
    return True


def test_ring_option_and_plan():
    d768 = scan_group_ring_plan(768, 8, 16, kp=KP_PLAIN, scan_group=4)
    assert len(d768["depths"]) >= 1 and d768["ring_depth"] in d768["depths"]
    for d in d768["depths"]:
        option_check("scan_group_ring", d)
        assert scan_group_ring_plan(768, 8, 16, kp=KP_PLAIN, scan_group=4, scan_group_ring=d)["ring_depth"] == d
        assert scan_group_ring_plan(768, 8, 16, kp=KP_PLAIN, scan_group=2, scan_group_ring=d)["ring_depth"] == d
        # launches without groups, and shapes with one depth, keep theirs whatever the value
        assert scan_group_ring_plan(768, 8, 16, kp=KP_PLAIN, scan_group=1, scan_group_ring=d)["ring_depth"] == \
            scan_plan(768, 8, 1 << 22, kp=KP_PLAIN)["ring_depth"]
        assert scan_group_ring_plan(768, 8, 1, kp=KP_PLAIN, scan_group=4, scan_group_ring=d)["ring_depth"] == \
            scan_plan(768, 8, 1 << 22, kp=KP_PLAIN)["ring_depth"]
        assert scan_group_ring_plan(384, 8, 16, kp=KP_PLAIN, scan_group=4, scan_group_ring=d)["ring_depth"] == \
            scan_plan(384, 8, 1 << 22, kp=KP_PLAIN)["ring_depth"]
        assert scan_group_ring_plan(100, 8, 16, kp=KP_PLAIN, scan_group=4, scan_group_ring=d)["ring_depth"] == \
            scan_plan(100, 8, 1 << 22, kp=KP_PLAIN)["ring_depth"]
    for bad in (-1, 1, 3, 5, 7, 64):
        if bad not in d768["depths"]:
            with pytest.raises(Exception):
                option_check("scan_group_ring", bad)
    with ScanIndex(16, 8, SZG_COSINE) as ix:
        ix.set_option("scan_group_ring", 0)
        with pytest.raises(Exception):
            ix.set_option("scan_group_ring", 5)


@pytest.mark.parametrize("dim,s,r,metric", CASES, ids=IDS)
def test_plain_handle_every_depth(dim, s, r, metric):
    """A plain 8-bit handle (three planes, norms summed at scan_norms = 1 and resident otherwise): answers and pass
    counts across scan_group_ring and scan_group; two queries per case against the oracle."""
    n = s * rows_per_step(dim) + r
    seed = SEED + dim * 1000 + s * 10 + (r % 7)
    rows = packed(seed, n, dim, 8)
    Q = orc.synth_vectors(seed + 1, 0, max(N_QUERIES), dim)
    want = list(POOL.map(lambda qi: orc.search_exact(rows, dim, 8, metric, Q[qi], k=K)[:2], (0, 2)))
    ref, passes = {}, {}
    configs = [(1, 0, 0), (2, 0, 0)] + [(4, d, nrm) for d in depths(dim) for nrm in (0, 1)] + \
              [(2, d, 0) for d in depths(dim)[1:]]
    with ScanIndex(dim, 8, metric) as ix:
        ix.synth(n, seed)
        assert (ix.read_rows(n - 1, 1) == rows[n - 1:]).all()
        for name, v in (("multi_query", 0), ("sketch", 0)):
            ix.set_option(name, v)
        for group, ring, norms in configs:
            for name, v in (("scan_group", group), ("scan_group_ring", ring), ("scan_norms", norms)):
                ix.set_option(name, v)
            for nq in N_QUERIES:
                ix.reset_stats()
                res = ix.search_topk(Q[:nq], K)
                st = ix.stats()
                what = (dim, n, "scan_group", group, "ring", ring, "norms", norms, "queries", nq)
                assert st["mq_queries"] == 0 and st["sketch_queries"] == 0 and st["scan_launches"] > 0, (what, st)
                if nq in ref:
                    assert same(res, ref[nq]), ("answers differ", what)
                else:
                    ref[nq] = res
                    for at, qi in enumerate((0, 2)):
                        assert [int(x) for x in res[0][qi, : res[2][qi]]] == [int(x) for x in want[at][0]], what
                        assert (res[1][qi, : res[2][qi]] == want[at][1]).all(), what
                key = (group, nq)
                count = (st["scan_launches"], st["scan_bytes"])
                assert passes.setdefault(key, count) == count, ("pass counts moved with the ring depth", what)
        if DEFAULT_TUNABLES:   # the grouped kernel served: a quarter of the passes of scan_group = 1 on a full launch
            assert passes[4, 16][1] * 4 == passes[1, 16][1]
            assert passes[2, 16][1] * 2 == passes[1, 16][1]


@pytest.mark.parametrize("dim,s,r,metric", CASES, ids=IDS)
def test_sketch_handle_every_depth(dim, s, r, metric):
    """A float32 handle through its 8-bit sketch (two planes, resident norms): answers, pass counts and the certificate
    trace's records across scan_group_ring; the records of one depth through cert_check (S and L)."""
    n = s * rows_per_step(dim) + r
    seed = SEED + 500000 + dim * 1000 + s * 10 + (r % 7)
    Q = orc.synth_vectors(seed + 1, 0, max(N_QUERIES), dim) * 0.7
    ref, passes, traces = {}, {}, {}
    with ScanIndex(dim, 32, metric) as ix:
        ix.synth(n, seed)
        for name, v in (("multi_query", 0), ("sketch", 1), ("sketch_min_rows", 1)):
            ix.set_option(name, v)
        ix.trace_certificates(True)
        for group, ring in [(1, 0)] + [(4, d) for d in depths(dim)] + [(2, d) for d in depths(dim)[1:]]:
            ix.set_option("scan_group", group)
            ix.set_option("scan_group_ring", ring)
            for nq in N_QUERIES:
                ix.reset_stats()
                res = ix.search_topk(Q[:nq], K)
                st = ix.stats()
                recs, ents, dropped = ix.certificates()
                what = (dim, n, "scan_group", group, "ring", ring, "queries", nq)
                assert dropped == 0 and st["sketch_queries"] + st["sketch_fallbacks"] == nq, (what, st)
                if nq in ref:
                    assert same(res, ref[nq]), ("answers differ", what)
                    assert recs.tobytes() == traces[nq][0].tobytes(), ("certificate records differ", what)
                    assert ents.tobytes() == traces[nq][1].tobytes(), ("certificate entries differ", what)
                else:
                    ref[nq], traces[nq] = res, (recs, ents)
                key = (group, nq)
                count = (st["scan_launches"], st["scan_bytes"], st["sketch_queries"], st["sketch_fallbacks"])
                assert passes.setdefault(key, count) == count, ("pass counts moved with the ring depth", what)
    # the records (the same at every depth) hold what they claim: S for the queries the sketch settled, L for the rest
    nq = N_QUERIES[0]
    recs, ents = traces[nq]
    corpus = cc.Corpus(packed(seed, n, dim, 32), dim, 32, metric)
    dists = np.stack(list(POOL.map(lambda q: orc.all_distances(corpus.packed, dim, 32, metric, q), Q[:nq])))
    summary = cc.check(corpus, Q[:nq], recs, ents, 0, dists=dists, what=("group ring", dim, n))
    assert summary.skipped == 0
    assert (recs["pass_"] == _lib.SZG_CERT_SKETCH).sum() == nq
