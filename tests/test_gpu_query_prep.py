"""Option query_prep: the queries of a top-k call through the sketch prepared on the card (kernels_query_prep.hip) by the
rule the host follows (csrc/query_prep.h).

1. Image and constants, host against card, byte for byte (ScanIndex.debug_query_prep, which goes through the search
   path's scaling and launch wrapper): both metrics, dimensions with a partial 16-element piece and partial plane words
   and the sweep's three step shapes, two and three digit planes, a float64 handle, batches of 1, 4, 33 and 64, and the
   vectors the rule can go wrong on (query_prep_cases.py).  At small dimensions the host form is also held to the rule
   as Python restates it.
2. The sweep cannot tell: the same call under query_prep 2 and 0, byte for byte on the certificate trace's sketch
   records and entries (rows, keys, bounds, distances, drop bound) and on the answers; under 2 the answers == the oracle.
3. The counters say which side ran; 4. refusals and bookkeeping.
"""
import threading

import numpy as np
import pytest
import torch   # (before the library loads its HIP runtime, as test_gpu_search_dev.py has it)

import oracle as orc
from syzgydb_amd import ScanIndex, SzgError, _lib
from syzgydb_amd.index import device_memory, option_check, query_prep_serves
import query_prep_cases as qpc
import test_gpu_sketch_matrix as tsm
import test_gpu_sketch_masked as tmk
import test_gpu_sketch_select as tss

pytestmark = pytest.mark.gpu

SEED = 0x53595A4700012000
EUC, COS = tsm.EUC, tsm.COS
MID = tsm.MID
DIMS = (1, 15, 16, 17, 64, 100, 384, 768)
BATCHES = (1, 4, 33, 64)


# ---- 1. image and constants --------------------------------------------------------------------------------------------

def assert_same_prep(ix, Q, what):
    """-> the host's (images, constants), which the card's equal byte for byte"""
    hi, hm = ix.debug_query_prep(Q, 0)
    ci, cm = ix.debug_query_prep(Q, 1)
    for j in range(Q.shape[0]):
        if hi[j].tobytes() != ci[j].tobytes():
            bad = np.flatnonzero(hi[j] != ci[j])
            raise AssertionError(("image bytes differ", what, "query", j, "first bytes", bad[:8], hi[j][bad[:8]], ci[j][bad[:8]]))
        assert hm[j].tobytes() == cm[j].tobytes(), ("constants differ (qnorm, m1, qscale, qconst, qnorm2)", what, "query", j,
                                                     [x.hex() for x in hm[j]], [x.hex() for x in cm[j]])
    return hi, hm


def assert_follows_the_rule(images, metas, Q, cosine, planes, gs, what):
    for j in range(Q.shape[0]):
        image, meta = qpc.prepare(Q[j], cosine, planes, gs)
        assert images[j].tobytes() == image, ("host image is not the rule's", what, j)
        assert [qpc.bits(float(x)) for x in metas[j]] == [qpc.bits(x) for x in meta], ("host constants", what, j, metas[j], meta)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", (COS, EUC), ids=["cos", "euc"])
def test_host_and_card_prepare_the_same_bytes(dim, metric):
    seed = SEED + dim
    with tsm.open_sketched(dim, metric) as ix:
        ix.synth(64, seed)
        for planes in (2, 3):
            ix.set_option("sketch_planes", planes)
            special = np.stack(list(qpc.vectors(dim, planes, seed).values()))
            what = ("prep", "dim", dim, MID[metric], "planes", planes)
            images, metas = assert_same_prep(ix, special, what + ("special",))
            gs = ix.sketch_info()["gscale"]
            assert (gs > 0) == (metric == EUC), (what, gs)
            if dim <= 100:
                assert_follows_the_rule(images, metas, special, int(metric == COS), planes, gs, what)
            for n in BATCHES:
                assert_same_prep(ix, qpc.batch(dim, planes, seed + n, n), what + ("batch", n))
            # the specials again at the end of a full batch: the last workgroups of a launch, the last slots of the buffers
            full = qpc.batch(dim, planes, seed + 7, 64)[::-1].copy()
            assert_same_prep(ix, full, what + ("reversed",))


@pytest.mark.parametrize("metric", (COS, EUC), ids=["cos", "euc"])
def test_float64_handle_prepares_the_same_bytes(metric):
    dim, n = 100, 64
    ix = ScanIndex(dim, 64, metric)
    with ix:
        for name, value in (("sketch_f64", 1), ("sketch", 1), ("sketch_min_rows", 1), ("multi_query", 0)):
            ix.set_option(name, value)
        ix.load(orc.synth_rows(SEED + 64, 0, n, dim, 64))
        for planes in (2, 3):
            ix.set_option("sketch_planes", planes)
            for nq in (13, 64):
                assert_same_prep(ix, qpc.batch(dim, planes, SEED + nq, nq), ("prep f64", MID[metric], planes, nq))


# ---- 2. the sweep cannot tell ------------------------------------------------------------------------------------------

def traced(ix, call, nq, what):
    """tss.traced_call for any call -> (answers, {query: (record bytes, entries' bytes, record, entries)}, prep stats)"""
    ix.certificates()
    ix.reset_stats()
    got = call()
    qp = ix.query_prep_stats()
    recs, ents, dropped = ix.certificates()
    assert dropped == 0, what
    out = {}
    for r in recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]:
        q = int(r["query"])
        assert q not in out, ("two sketch records of one query", what, q)
        e = ents[int(r["first_entry"]): int(r["first_entry"]) + int(r["n_entries"])]
        out[q] = (b"".join(r[f].tobytes() for f in tss.REC_FIELDS), e.tobytes(), r, e)
    assert sorted(out) == list(range(nq)), ("one sketch record per query", what)
    return got, out, qp


def assert_same_under_prep(ix, call, nq, what):
    """The call under query_prep 2 and 0: records, drop bound, entries and answers byte for byte; the counters name the
    side.  -> the answers under 2"""
    seen = {}
    for opt in (2, 0):
        ix.set_option("query_prep", opt)
        seen[opt] = traced(ix, call, nq, what + ("query_prep", opt))
    ix.set_option("query_prep", 2)
    (g2, t2, s2), (g0, t0, s0) = seen[2], seen[0]
    assert s2["queries_dev"] == nq and s2["queries_host"] == 0 and s2["launches"] >= 1, (what, s2)
    assert s0 == {"queries_dev": 0, "queries_host": nq, "launches": 0}, (what, s0)
    for q in range(nq):
        r2, r0 = t2[q][2], t0[q][2]
        assert r2["thr_min"].tobytes() == r0["thr_min"].tobytes(), ("drop bound / lb differs", what, q, r2["thr_min"], r0["thr_min"])
        assert int(r2["n_entries"]) == int(r0["n_entries"]), ("entry counts differ", what, q)
        e2, e0 = t2[q][3], t0[q][3]
        assert (e2["row"] == e0["row"]).all(), ("rows differ", what, q, e2["row"], e0["row"])
        assert e2["key"].tobytes() == e0["key"].tobytes(), ("keys differ", what, q)
        assert t2[q][1] == t0[q][1], ("entries differ (bounds, distances)", what, q)
        assert t2[q][0] == t0[q][0], ("records differ", what, q, r2, r0)
    for a, b in zip(g2, g0):
        assert a.tobytes() == b.tobytes(), ("answers differ", what)
    return g2


def queries(seed, nq, dim):
    return orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7


# (name, dim, metric, rows, queries, k, options): rows at 17, one tile - 1 and + 1, one step of the launch + 77 + 77; the
# one-block, wide and shared launches forced at 1, 16, 17, 33 and 64 queries; the three step shapes; Euclid: gs > 0
def _big(dim):
    return tsm.n_rows_of(dim, "s1") + 77


PLAIN = [
    ("rows17", 64, COS, 17, 3, 10, {}),
    ("tile-1", 384, EUC, 15, 16, 10, {}),
    ("tile+1", 768, COS, 17, 17, 1, {"sketch_list": 8}),
    ("step", 64, EUC, "big", 40, 10, {}),
    ("step768", 768, EUC, "big", 5, 10, {}),
    ("forced-q1", 384, COS, "big", 1, 10, {"sketch_wide": 2, "sketch_share": 2}),
    ("forced-q16", 64, EUC, "big", 16, 10, {"sketch_wide": 2, "sketch_share": 2}),
    ("forced-q17", 768, COS, "big", 17, 10, {"sketch_wide": 2, "sketch_share": 2}),
    ("forced-q33", 384, EUC, "big", 33, 10, {"sketch_wide": 2, "sketch_share": 2}),
    ("forced-q64", 768, COS, "big", 64, 10, {"sketch_wide": 2, "sketch_share": 2}),
    ("forced-q64-tile", 64, COS, 17, 64, 1, {"sketch_wide": 2, "sketch_share": 2, "sketch_list": 8}),
]


@pytest.mark.parametrize("case", PLAIN, ids=[c[0] for c in PLAIN])
def test_same_trace_and_answers(case):
    name, dim, metric, rows, nq, k, options = case
    n = _big(dim) if rows == "big" else rows
    seed = SEED + dim * 100 + (n % 1000) + k
    packed = tsm.synth_corpus(seed, n, dim)
    Q = queries(seed, nq, dim)
    what = ("query_prep", name, "rows", n)
    with tsm.open_sketched(dim, metric, **options) as ix:
        ix.synth(n, seed)
        got = assert_same_under_prep(ix, lambda: ix.search_topk(Q, k), nq, what)
        tsm.assert_answers(got, packed, dim, metric, Q, k, None, what)
        st = ix.stats()
        assert st["sketch_queries"] + st["sketch_fallbacks"] == nq, (what, st)


def test_same_under_masks_two_different_in_the_batch():
    dim, metric, nq, k = 64, COS, 17, 10
    n = _big(dim)
    seed = SEED + 9100
    packed = tsm.synth_corpus(seed, n, dim)
    Q = queries(seed, nq, dim)
    rng = np.random.default_rng(seed)
    a, b = rng.random(n) < 0.7, rng.random(n) < 0.4
    el = np.stack([a if j % 2 == 0 else b for j in range(nq)])
    what = ("query_prep", "masked", n)
    with tmk.open_masked(dim, metric) as ix:
        ix.synth(n, seed)
        got = assert_same_under_prep(ix, lambda: ix.search_topk(Q, k, allow=el), nq, what)
        tmk.assert_answers_per_query(got, tsm.cc.Corpus(packed, dim, 32, metric), Q, k, el, what)
        assert ix.sketch_masked_info()["launches"] >= 1, what


def test_same_on_two_shards_of_one_device():
    dim, metric, nq, k = 64, EUC, 20, 10
    n = _big(dim)
    seed = SEED + 9200
    packed = tsm.synth_corpus(seed, n, dim)
    Q = queries(seed, nq, dim)
    what = ("query_prep", "devices 0, 0", n)
    with tsm.open_sketched(dim, metric, devices=[0, 0]) as ix:
        ix.synth(n, seed)
        got = assert_same_under_prep(ix, lambda: ix.search_topk(Q, k), nq, what)
        if tsm.DEFAULT_TUNABLES:   # (a call of 20 is one batch: one launch of the preparing kernel per shard)
            ix.reset_stats()
            ix.search_topk(Q, k)
            assert ix.query_prep_stats() == {"queries_dev": nq, "queries_host": 0, "launches": 2}
        tsm.assert_answers(got, packed, dim, metric, Q, k, None, what)


def test_same_with_a_tombstone_among_the_first_k():
    dim, metric, nq, k = 64, COS, 9, 10
    n = _big(dim)
    seed = SEED + 9300
    packed = tsm.synth_corpus(seed, n, dim)
    Q = queries(seed, nq, dim)
    what = ("query_prep", "tombstone", n)
    with tsm.open_sketched(dim, metric) as ix:
        ix.synth(n, seed)
        ix.tombstone_rows([3, n - 1])
        el = np.ones(n, dtype=bool)
        el[[3, n - 1]] = False
        got = assert_same_under_prep(ix, lambda: ix.search_topk(Q, k), nq, what)
        tsm.assert_answers(got, packed, dim, metric, Q, k, el, what)


@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_same_from_a_device_tensor(dtype):
    dim, metric, nq, k = 64, COS, 12, 10
    n = _big(dim)
    seed = SEED + 9400
    packed = tsm.synth_corpus(seed, n, dim)
    t = torch.from_numpy(queries(seed, nq, dim)).to(getattr(torch, dtype)).cuda()
    Q = t.to(torch.float64).cpu().numpy()   # (the widening is exact)
    what = ("query_prep", "tensor", dtype)
    with tsm.open_sketched(dim, metric) as ix:
        ix.synth(n, seed)
        got = assert_same_under_prep(ix, lambda: ix.search_topk_tensor(t, k), nq, what)
        host = ix.search_topk(Q, k)   # (under 2)
        for x, y in zip(got, host):
            assert x.tobytes() == y.tobytes(), ("tensor and host-array answers differ", what)
        tsm.assert_answers(got, packed, dim, metric, Q, k, None, what)


def test_four_threads_of_lone_searches():
    dim, metric, k, per = 64, COS, 10, 6
    n = _big(dim)
    seed = SEED + 9500
    packed = tsm.synth_corpus(seed, n, dim)
    Q = queries(seed, 4 * per, dim)
    with tsm.open_sketched(dim, metric) as ix:
        ix.synth(n, seed)
        ix.trace_certificates(False)
        ix.search_topk(Q[0], k)   # (the sketch is built before the threads start)
        answers = {}
        for opt in (2, 0):
            ix.set_option("query_prep", opt)
            ix.reset_stats()
            out = [None] * len(Q)
            errors = []

            def work(t):
                try:
                    for i in range(t * per, (t + 1) * per):
                        out[i] = ix.search_topk(Q[i], k)
                except Exception as e:   # noqa: BLE001 -- reported below, on the test's thread
                    errors.append(e)

            threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
            for th in threads:
                th.start()
            for th in threads:
                th.join()
            assert not errors, errors
            qp = ix.query_prep_stats()
            side, other = ("queries_dev", "queries_host") if opt == 2 else ("queries_host", "queries_dev")
            assert qp[side] == len(Q) and qp[other] == 0, (opt, qp)
            answers[opt] = out
        for i in range(len(Q)):
            for x, y in zip(answers[2][i], answers[0][i]):
                assert x.tobytes() == y.tobytes(), ("answers differ", i)
            tsm.assert_answers(answers[2][i], packed, dim, metric, Q[i: i + 1], k, None, ("threads", i))


# ---- 3. the counters ---------------------------------------------------------------------------------------------------

def test_counters_follow_the_batch_rule():
    dim, metric, k = 64, COS, 10
    n = _big(dim)
    seed = SEED + 9600
    serves1, least = query_prep_serves(1, 1)
    assert not serves1 and least >= 2
    assert query_prep_serves(1, least)[0] and not query_prep_serves(1, least - 1)[0]
    assert query_prep_serves(2, 1)[0] and not query_prep_serves(0, 64)[0]
    Q = queries(seed, 40, dim)
    with tsm.open_sketched(dim, metric) as ix:
        ix.synth(n, seed)
        ix.trace_certificates(False)
        ix.set_option("query_prep", 1)
        ix.reset_stats()
        ix.search_topk(Q[: least - 1], k)
        assert ix.query_prep_stats() == {"queries_dev": 0, "queries_host": least - 1, "launches": 0}
        ix.reset_stats()
        ix.search_topk(Q, k)
        qp = ix.query_prep_stats()
        assert qp["queries_dev"] + qp["queries_host"] == 40, qp
        if tsm.DEFAULT_TUNABLES:   # a call of 40: batches of 4, 16, 16, 4 (sketch_plan.h)
            batches = [4, 16, 16, 4]
            dev = sum(b for b in batches if query_prep_serves(1, b)[0])
            assert qp == {"queries_dev": dev, "queries_host": 40 - dev, "launches": sum(1 for b in batches if query_prep_serves(1, b)[0])}, qp
        ix.set_option("query_prep", 2)
        ix.search_topk(Q[:5], k)
        assert ix.query_prep_stats()["queries_dev"] >= 5
        ix.reset_stats()
        assert ix.query_prep_stats() == {"queries_dev": 0, "queries_host": 0, "launches": 0}


# ---- 4. refusals and bookkeeping ---------------------------------------------------------------------------------------

def test_refusals_and_memory():
    for value in (0, 1, 2):
        option_check("query_prep", value)
    for value in (-1, 3, 100):
        with pytest.raises(SzgError) as e:
            option_check("query_prep", value)
        assert "query_prep is 0, 1 or 2" in str(e.value)
    dim = 64
    blocks0, bytes0 = device_memory()
    with ScanIndex(dim, 32, COS) as ix:   # (sketch = 0: the handle keeps none)
        ix.set_option("sketch", 0)
        ix.synth(100, SEED)
        with pytest.raises(SzgError) as e:
            ix.set_option("query_prep", 3)
        assert "query_prep is 0, 1 or 2" in str(e.value)
        for on_card in (0, 1):
            with pytest.raises(SzgError) as e:
                ix.debug_query_prep(np.ones((2, dim)), on_card)
            assert e.value.code == _lib.SZG_E_UNSUPPORTED, e.value
    with ScanIndex(dim, 8, COS) as ix:    # (a plain 8-bit handle: its queries are the host's, whatever the option)
        ix.synth(100, SEED)
        ix.set_option("query_prep", 2)
        with pytest.raises(SzgError) as e:
            ix.debug_query_prep(np.ones((2, dim)), 1)
        assert e.value.code == _lib.SZG_E_UNSUPPORTED, e.value
        ix.search_topk(np.ones((3, dim)), 5)
        assert ix.query_prep_stats() == {"queries_dev": 0, "queries_host": 0, "launches": 0}
    with tsm.open_sketched(dim, COS) as ix:
        ix.synth(1000, SEED)
        ix.set_option("query_prep", 2)
        ix.search_topk(queries(SEED, 20, dim), 10)
        ix.debug_query_prep(np.ones((100, dim)), 1)   # (more than one context's batch: the hook goes in pieces)
        assert device_memory()[0] > blocks0
    assert device_memory() == (blocks0, bytes0), "device blocks outlive their handles"
