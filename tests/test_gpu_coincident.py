"""Keys at and near zero: queries that coincide with stored rows, under every sweep's certificates.

tests/test_gpu_certificates.py checks the chain K / L / C / S (and K_s, L_s, D, C_s, T, S_r with the sketch state) against
float64 / long double for queries far from every row.  Here the queries sit ON rows and within a few float32 spacings
of them (coincident_cases.py: P0, P1, P2, four byte-identical rows at distance 0, a corpus shifted by +1 000, queries
parallel to a row under cosine) -- "more like this document", where a float32 distance cancels completely.  The corpora
are small on purpose: up to cert_check.WIDE_LIMIT (query, row, element) triples the reference forms every key element by
element, with an error relative to the key.

Per case: top-k at k = 1, 4 and 10 (fewer, as many and more than the rows at distance 0: the oracle's order among equal
distances) and radius searches, lone and as a batch, at five radii -- the smallest positive double (a radius of 0 means
"no radius" to the reference and the library refuses it: that refusal is asserted), the oracle's float64 distance of the
near row (<= includes it), np.nextafter of it towards 0 (excludes it), 1e-12 and one that takes some thirty rows --
every answer against orc.search_exact, every record through cert_check.check; then the same calls under a resident mask
that keeps the planted rows, and with one of the four equal rows tombstoned.

Conditions of every call (not measurements): no candidate is skipped (the corpora hold no non-finite element and no zero
row); every planted (query, row) pair whose row is eligible is among the keyed entries K or K_s checked -- a test that
never looked at the pair it exists for would pass; on the one-sweep Euclidean legs of 32- and 16-bit rows the recorded
float32 key of P0 and P1 is exactly 0 while P1's real-number key is positive: the test stands on the gap that
key_bound.h's 4 u^2 |g|^2 closes.

Families, forced by options and confirmed from the statistics and the records' pass kinds and sweeps: the one-sweep
kernel (every width, the smallest row-shape cell and the smallest ragged class of the lattice); the int8 shared sweep;
the bfloat16 shared sweeps, staged and direct, in their three tails; the sketch pre-pass in its forms.  No option
reaches the plain float32 shared sweep any more (szg_index::mq_bf16 is a constant 1), so that family has no leg.

MARGINS keeps the largest |key - real| / eps of this file's calls (scripts/dev_certificates.py writes them out and
fails on a ratio above 1; cert_check.check asserts every bound as it goes).
"""
import numpy as np
import pytest

import coincident_cases as cases
import oracle as orc
import scan_lattice as lat
import test_gpu_certificates as tgc
import test_gpu_sketch_matrix as tsm
import test_gpu_sketch_share as tss
import test_gpu_sketch_wide as tsw
from syzgydb_amd import SzgError, _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import scan_collect_plan, scan_masked_plan, scan_matrix_plan

pytestmark = pytest.mark.gpu

METRICS = (0, 1)
MID = {0: "euc", 1: "cos"}
MARGINS = cc.Margins()
KS = (1, 4, 10)
TOPK_PASSES = (_lib.SZG_CERT_TOPK, _lib.SZG_CERT_ESCALATION)
COLLECT_PASSES = (_lib.SZG_CERT_RADIUS_SINGLE, _lib.SZG_CERT_RADIUS_SHARED, _lib.SZG_CERT_SKETCH_RADIUS)


def sketch_state(ix, case):
    """(Corpus of the sketch bytes, gscale, exception rows) of a handle with a sketch in step with its rows, else None."""
    info = ix.sketch_info()
    if not (info["exists"] and info["in_sync"]):
        return None
    rows = ix.sketch_rows()[0]
    kept = getattr(case, "_sk", None)   # (the same bytes call after call: keep the Corpus and with it the keys it computed)
    if kept is None or kept.metric != case.corpus.metric or not np.array_equal(kept.packed, rows):
        kept = case._sk = cc.Corpus(rows, case.corpus.dim, 8, case.corpus.metric)
    return kept, info["gscale"], info["exc_rows"]


def eligible_2d(eligible, nq, n):
    return np.broadcast_to(np.ones(n, dtype=bool) if eligible is None else np.asarray(eligible, dtype=bool), (nq, n))


def assert_pairs_checked(case, recs, ents, eligible, passes, what, queries=None, radii=None):
    """Every planted (query, row) pair with an eligible row -- radii: whose oracle distance is within the query's radius,
    so that the answer must contain it -- is among the keyed entries of a record K or K_s checked."""
    el = eligible_2d(eligible, case.Q.shape[0], case.corpus.n)
    for qi, row in case.pairs:
        if not el[qi, row] or (queries is not None and qi not in queries) or np.isnan(case.dists()[qi, row]):
            continue   # (a NaN distance -- the reference's unclamped acos at a parallel pair -- is never a neighbour)
        if radii is not None and not case.dists()[qi, row] <= radii[qi]:
            continue
        at = qi if queries is None else queries.index(qi)
        seen = set()
        for rec in recs[recs["query"] == at]:
            p = int(rec["pass_"])
            if p in passes or (p == _lib.SZG_CERT_SKETCH and np.isfinite(rec["thr_min"])):
                e = ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]
                seen.update(int(x) for x in e["row"][(e["flags"] & _lib.SZG_CERT_ENTRY_NO_KEY) == 0])
        assert row in seen, ("a planted pair was never under K", what, "query", qi, "row", row)


def topk(ix, case, k, what, eligible=None, pairs=True, **filt):
    """One top-k call: K, L (C, S, K_s, L_s, D) on its records, A on its answers.  -> (records, entries)"""
    corpus, Q = case.corpus, case.Q
    r, d, cnt = ix.search_topk(Q, k, **filt)
    recs, ents, dropped = ix.certificates()
    dists = sketch = None
    if (recs["pass_"] == _lib.SZG_CERT_SKETCH).any():
        dists, sketch = case.dists(), sketch_state(ix, case)
    what = what + ("k", k)
    s = cc.check(corpus, Q, recs, ents, dropped, eligible=eligible, dists=dists, margins=MARGINS, what=what, sketch=sketch)
    assert s.skipped == 0, ("candidates without a bound on a corpus that plants none", what, sorted(s.skipped_rows)[:8])
    first = recs[(recs["pass_"] == _lib.SZG_CERT_TOPK) | ((recs["pass_"] == _lib.SZG_CERT_SKETCH) & (recs["certified"] == 1))]
    assert sorted(int(x) for x in first["query"]) == list(range(Q.shape[0])), ("one first-pass record per query", what)
    if pairs:
        assert_pairs_checked(case, recs, ents, eligible, TOPK_PASSES, what)
    el = eligible_2d(eligible, Q.shape[0], corpus.n)
    for qi in range(Q.shape[0]):
        want = orc.search_exact(corpus.packed, corpus.dim, corpus.bits, corpus.metric, Q[qi], k=k,
                                allow=None if eligible is None else el[qi].astype(np.uint8))[:2]
        tgc.assert_same(r[qi, : cnt[qi]], d[qi, : cnt[qi]], want, what + ("query", qi))
        assert cnt[qi] == len(want[0]), ("count differs", what, qi)
    return recs, ents


def radius(ix, case, kind, what, eligible=None, lone=False, pairs=True, room=False, **filt):
    """Radius searches at RADIUS_KINDS[kind], one batch or (lone) one call per planted query: the hits against the
    oracle, C (C_s, T, S_r, K_s with the sketch state) and K on the records.  room: the batch gets buffers for every row
    of every query, as test_gpu_certificates.traced_radius_all gives them -- far from the origin a shared sweep's
    absolute bound puts every row under the threshold, and a query with more hits than its share of the first buffers
    would be swept again on its own, leaving no record of the shared sweep.  -> [(records, entries)] per call"""
    corpus, Q = case.corpus, case.Q
    radii = case.radii(kind, eligible)
    what = what + ("radius", cases.RADIUS_KINDS[kind], "lone" if lone else "batch")
    el = eligible_2d(eligible, Q.shape[0], corpus.n)
    calls = [[qi] for qi in sorted({qi for qi, _ in case.pairs})] if lone else [list(range(Q.shape[0]))]
    out = []
    for qs in calls:
        if lone:
            got = [ix.search_radius(Q[qs[0]], float(radii[qs[0]]), **filt)]
        elif room:
            full = Q.shape[0] * corpus.n
            ix.trace_certificates(False)   # (the first batch on a context grows the buffers: RadiusCall::finish)
            ix.search_radius_batch(Q, radii, capacity=full, **filt)
            ix.trace_certificates(True)
            got = ix.search_radius_batch(Q, radii, capacity=full, **filt)
        else:
            got = ix.search_radius_batch(Q, radii, **filt)
        recs, ents, dropped = ix.certificates()
        sketch = sketch_state(ix, case) if (recs["pass_"] == _lib.SZG_CERT_SKETCH_RADIUS).any() else None
        s = cc.check(case.lone if lone else corpus, Q[qs], recs, ents, dropped, eligible=None if eligible is None else el[qs],
                     dists=case.dists()[qs], margins=MARGINS, what=what + ("queries", qs[0], "..."), sketch=sketch, radii=radii[qs])
        assert s.skipped == 0, ("candidates without a bound on a corpus that plants none", what, sorted(s.skipped_rows)[:8])
        assert sorted(int(x) for x in recs["query"]) == list(range(len(qs))), ("one collect record per query", what, recs["query"])
        for i, qi in enumerate(qs):
            want = orc.search_exact(corpus.packed, corpus.dim, corpus.bits, corpus.metric, Q[qi], radius=float(radii[qi]),
                                    allow=None if eligible is None else el[qi].astype(np.uint8))[:2]
            tgc.assert_same(got[i][0], got[i][1], want, what + ("query", qi, "radius", float(radii[qi])))
        if pairs:
            # at every radius: a planted pair whose row the answer must contain is among the entries K (K_s) checked --
            # the four rows at distance 0 at the smallest radius, every planted row at its own distance and at the
            # ordinary radius; the radius just under the near row's distance excludes it (the oracle's answer, above)
            assert_pairs_checked(case, recs, ents, eligible, COLLECT_PASSES, what, queries=qs, radii=radii)
        if kind == 1 and pairs:
            for i, qi in enumerate(qs):
                assert len(got[i][0]) >= 1, ("the near row is not within its own distance", what, qi)
        out.append((recs, ents))
    return out


def legs(ix, case, what, eligible=None, ks=KS, lone=True, room=False, **filt):
    """The calls of one state of a handle.  -> {("topk", k) | ("radius", kind, lone): records}"""
    out = {}
    for k in ks:
        out["topk", k] = topk(ix, case, k, what, eligible, **filt)
    for kind in range(len(cases.RADIUS_KINDS)):
        out["radius", kind, False] = radius(ix, case, kind, what, eligible, room=room, **filt)
        if lone:
            out["radius", kind, True] = radius(ix, case, kind, what, eligible, lone=True, **filt)
    return out


def three_states(ix, case, what, confirm, **kw):
    """Plain, under a resident mask that keeps the planted rows, and with one of the rows at distance 0 tombstoned."""
    with pytest.raises(SzgError, match="radius must be > 0"):
        ix.search_radius(case.Q[0], 0.0)
    confirm(legs(ix, case, what, **kw))
    allow = case.keep_mask()
    with ix.mask(allow) as m:
        confirm(legs(ix, case, what + ("resident mask",), allow, masks=m, **kw))
    dead = np.zeros(case.corpus.n, dtype=bool)
    dead[case.copies[1]] = True
    assert ix.tombstone_rows(np.flatnonzero(dead)) == 1
    confirm(legs(ix, case, what + ("tombstone",), ~dead, **kw))


def all_records(out, name):
    return [recs for key, got in out.items() if key[0] == name
            for recs in ([got[0]] if name == "topk" else [r for r, _ in got])]


def confirm_sweeps(topk_keys, topk_sweep, batch_pass, batch_sweep):
    """-> a check of legs()' records: the first top-k passes carry `topk_keys` and `topk_sweep`, radius batches are
    `batch_pass` records of `batch_sweep`, lone radius calls one-sweep collects."""
    def confirm(out):
        for recs in all_records(out, "topk"):
            first = tgc.first_pass(recs)
            assert set(int(x) for x in first["keys"]) <= set(topk_keys) and (first["sweep"] == topk_sweep).all(), (first["keys"], first["sweep"])
        for key, got in out.items():
            if key[0] == "radius":
                for recs, _ in got:
                    want = (_lib.SZG_CERT_RADIUS_SINGLE, 0) if key[2] else (batch_pass, batch_sweep)
                    assert (recs["pass_"] == want[0]).all() and (recs["sweep"] == want[1]).all(), (key, recs["pass_"], recs["sweep"])
    return confirm


# ---- the one-sweep kernel -----------------------------------------------------------------------------------------------------

def one_sweep_cells():
    out = []
    for bits in lat.WIDTHS:
        cs = lat.cells(bits)
        shapes = [c for c in cs if c.kind == "shape"]
        if shapes:
            out.append((min(shapes, key=lambda c: c.dim), False))
        out.append((min((c for c in cs if c.kind == "class" and c.cls[3] == "ragged"), key=lambda c: c.dim), False))
    out += [(c, True) for c, _ in list(out) if c.bits >= 32 and c.kind == "class"]   # far from the origin
    return out


ONE_SWEEP = [(c, far, m) for c, far in one_sweep_cells() for m in METRICS]


@pytest.mark.parametrize("cell,far,metric", ONE_SWEEP,
                         ids=["%s%s-%s" % (lat.cell_id(c), "-far" if f else "", MID[m]) for c, f, m in ONE_SWEEP])
def test_one_sweep_kernel(cell, far, metric):
    """multi_query = 0, sketch = 0: every search is the one-sweep kernel's, top-k lists and collect sweeps."""
    case = cases.build(cell.bits, cell.dim, 8, metric, qmax=cases.QMAX_ONE_SWEEP.get(cell.bits), far=far)
    what = ("one-sweep", lat.cell_id(cell), "far" if far else "near", MID[metric])
    confirm = confirm_sweeps((_lib.SZG_CERT_KEYS_SINGLE,), 0, _lib.SZG_CERT_RADIUS_SINGLE, 0)
    with tgc.open_index(case.corpus, multi_query=0, sketch=0) as ix:
        if metric == 0 and cell.bits in (16, 32):
            recs, ents = topk(ix, case, 1, what + ("the gap",))
            real, _ = case.corpus.keys(case.Q)
            for qi, row, kind in case.planted[:2]:
                rec = tgc.first_pass(recs)[tgc.first_pass(recs)["query"] == qi][0]
                e = ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]
                key = e["key"][e["row"] == row]
                assert key.size == 1 and key[0] == 0.0, ("the float32 key of a query that rounds to the row is 0", what, kind, key)
                assert (real[qi, row] > 0.0) == (kind == "P1"), (what, kind, real[qi, row])
        three_states(ix, case, what, confirm)
        tgc.assert_scan_kernel_served(ix)


# ---- the shared sweeps --------------------------------------------------------------------------------------------------------

I8 = [(bits, dim, m) for bits, dims in ((8, (192, 100)), (4, (384, 200))) for dim in dims for m in METRICS]


@pytest.mark.parametrize("bits,dim,metric", I8, ids=["%db-d%d-%s" % (b, d, MID[m]) for b, d, m in I8])
def test_int8_shared_sweep(bits, dim, metric):
    """16 queries through mq_score_i8s_kernel (whole 64-byte steps) and mq_score_i8_kernel (a ragged row)."""
    case = cases.build(bits, dim, 16, metric, qmax=cases.QMAX_SHARED)
    what = ("int8", bits, dim, MID[metric])
    with tgc.open_index(case.corpus, sketch=0, contexts=1) as ix:
        three_states(ix, case, what, confirm_sweeps((_lib.SZG_CERT_KEYS_SHARED_INT8,), 1, _lib.SZG_CERT_RADIUS_SHARED, 1))
        st = ix.stats()
        assert st["mq_queries"] > 0 and st["mq_bf16_sweeps"] == 0, st


TAILS = (({}, _lib.SZG_CERT_KEYS_BF16_BAND), ({"force_no_refine": 1}, _lib.SZG_CERT_KEYS_BF16_RESCORED),
         ({"force_matrix": 1}, _lib.SZG_CERT_KEYS_SHARED_BF16))


def bf16_tails(ix, case, what, radius_sweep, far=False):
    """The three tails of a bfloat16 shared sweep at k = 1, 4 and 10 (the sweep's own keys also under the tight check),
    then the three states in the default tail with the radius batches."""
    seen = set()
    for options, want in TAILS:
        for name, value in options.items():
            ix.set_option(name, value)
        for k in KS:
            recs, ents = topk(ix, case, k, what + (cc.KEYS_NAMES[want],))
            first = tgc.first_pass(recs)
            kinds = set(int(x) for x in first["keys"])
            # (as test_gpu_certificates.bf16_forms at 17 dimensions and more: every tail is the one asked for, no batch
            # is redone through the score matrix -- but on 8-bit rows here: 64 queries over 1 621 rows put more
            # candidates into a query's error band than the refine launch takes, and some calls are redone)
            assert kinds == {want} or (case.corpus.bits == 8 and kinds <= {want, _lib.SZG_CERT_KEYS_SHARED_BF16}), (
                what, first["keys"], ix.stats())
            assert (first["sweep"] == 2).all(), (what, first["sweep"])
            band = first[first["keys"] != _lib.SZG_CERT_KEYS_SHARED_BF16]
            assert np.isfinite(band["thr_min"]).all()   # L held for the threshold (and the band's edge): they entered thr_min
            if _lib.SZG_CERT_KEYS_SHARED_BF16 in kinds:
                assert cc.check_bf16_tight(case.corpus, case.Q, recs, ents, MARGINS, what) > 0
            seen |= kinds
        for name in options:
            ix.set_option(name, 0)
    assert len(seen) == 3 and case.corpus.dim >= 17, (what, seen)
    st = ix.stats()
    nq = case.Q.shape[0]
    redo = case.corpus.bits == 8   # (a call redone through the matrix sweeps twice)
    assert st["mq_bf16_sweeps"] >= 3 * len(KS) and st["mq_queries"] >= 3 * len(KS) * nq, st
    assert redo or (st["mq_bf16_sweeps"] == 3 * len(KS) and st["mq_queries"] == 3 * len(KS) * nq), st   # one sweep per call so far

    def confirm(out):
        confirm_sweeps([w for _, w in TAILS], 2, _lib.SZG_CERT_RADIUS_SHARED, radius_sweep)(out)
        if radius_sweep == 2:
            for recs, ents in (out["radius", kind, False][0] for kind in range(len(cases.RADIUS_KINDS))):
                cc.check_bf16_tight(case.corpus, case.Q, recs, ents, MARGINS, what)
    three_states(ix, case, what, confirm, room=far)
    st = ix.stats()
    # three states of len(KS) top-k calls and five radius batches each (a radius batch that finds its hit buffers short
    # is searched a second time: at least one sweep each)
    shared = 3 * (len(KS) + len(cases.RADIUS_KINDS))
    assert st["mq_bf16_sweeps"] >= 3 * len(KS) + (shared if radius_sweep == 2 else 3 * len(KS)), st
    assert st["mq_queries"] >= (3 * len(KS) + shared) * nq, st


BF16S = [(bits, dim, far, m) for bits, dims in ((32, (17, 40)), (64, (17, 24))) for dim in dims for far in (False, True)
         for m in METRICS if not far or dim > 17]


@pytest.mark.parametrize("bits,dim,far,metric", BF16S,
                         ids=["%db-d%d%s-%s" % (b, d, "-far" if f else "", MID[m]) for b, d, f, m in BF16S])
def test_bf16_staged_sweep(bits, dim, far, metric):
    """mq_score_bf16s_kernel on 32- and 64-bit rows, 16 queries; far: the corpus and the queries 1 000 from the origin,
    where the expanded form's |x|^2 is 10^6 times the keys at the planted rows."""
    case = cases.build(bits, dim, 16, metric, far=far)
    with tgc.open_index(case.corpus, sketch=0, contexts=1) as ix:
        bf16_tails(ix, case, ("bf16s", bits, dim, "far" if far else "near", MID[metric]), 2, far=far)


BF16D = [(16, dim, 16, m) for dim in (17, 40) for m in METRICS] + [(8, 192, 64, m) for m in METRICS]


@pytest.mark.parametrize("bits,dim,nq,metric", BF16D, ids=["%db-d%d-q%d-%s" % (b, d, q, MID[m]) for b, d, q, m in BF16D])
def test_bf16_direct_sweeps(bits, dim, nq, metric):
    """mq_score_bf16d_kernel (16-bit rows) and mq_score_bf16d8_kernel (tiled 8-bit rows, more than 48 queries; their
    radius batches stay on the int8 sweep: a radius is the threshold)."""
    case = cases.build(bits, dim, nq, metric, qmax=cases.QMAX_SHARED if bits == 8 else None)
    with tgc.open_index(case.corpus, sketch=0, contexts=1) as ix:
        bf16_tails(ix, case, ("bf16d", bits, dim, nq, MID[metric]), 2 if bits == 16 else 1)


# ---- the sketch pre-pass --------------------------------------------------------------------------------------------------------

def head(case, nq):
    sub = cases.Case(case.corpus, case.Q[:nq], case.planted, case.copies, case.r0)
    sub._dists = case.dists()[:nq]
    return sub


def sketch_topk(ix, case, what, want_passes, eligible=None, ks=KS, **filt):
    """Top-k calls through the sketch; want_passes: the sketch sweeps' passes over the rows per call (None: not known),
    under the rule of test_gpu_sketch_matrix.assert_pass_count.  -> queries the sketch settled"""
    settled = 0
    for k in ks:
        ix.reset_stats()
        recs, _ = topk(ix, case, k, what, eligible, **filt)
        st = ix.stats()
        sk = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]
        assert sorted(int(x) for x in sk["query"]) == list(range(case.Q.shape[0])), ("one sketch record per query", what)
        assert st["sketch_queries"] + st["sketch_fallbacks"] == case.Q.shape[0] and st["mq_queries"] == 0, (what, st)
        if want_passes is not None:
            tsm.assert_pass_count(st, case.corpus.n, case.corpus.dim, case.Q.shape[0], want_passes, what + ("k", k))
        settled += int((sk["certified"] == 1).sum())
    return settled


SKETCH = [(dim, far, m) for dim, far in ((64, False), (100, False), (64, True)) for m in METRICS]


def lone_cases(case):
    """One one-query Case per planted query (its calls take the one-query kernel)."""
    out = []
    for qi in sorted({q for q, _, _ in case.planted}):
        one = cases.Case(case.lone, case.Q[qi:qi + 1], [(0, row, kind) for q, row, kind in case.planted if q == qi],
                         case.copies if qi == 0 else (), case.r0)
        one._dists = case.dists()[qi:qi + 1]
        out.append((qi, one))
    return out


@pytest.mark.parametrize("dim,far,metric", SKETCH, ids=["d%d%s-%s" % (d, "-far" if f else "", MID[m]) for d, f, m in SKETCH])
def test_sketch_pre_pass(dim, far, metric):
    """float32 rows behind their 8-bit sketch (sketch = 1, sketch_min_rows = 1): lone calls (the one-query kernel), 16
    queries under sketch_matrix 1 (the grouped kernels) and 0 (the matrix sweep), 32 under sketch_wide = 2, 136 under
    sketch_share = 2 (64 dimensions: 100 would pass the reference's limit), radius searches through the sketch lone and
    as a batch of 16, and the masked forms under one shared mask and under tombstones.  Rows of 100 bytes are not tiled:
    the plan hooks say that no matrix form serves them, and every call there takes the one-query and grouped kernels.
    far: the corpus and the queries 1 000 from the origin -- under Euclid every row lies within a step of the sketch's one
    scale, under cosine within 1e-3 of one direction; the sketch may settle nothing there, its claims (K_s, L_s, D, T,
    S_r) and the answers are asked all the same."""
    nq_all = 136 if dim == 64 else 32
    case = cases.build(32, dim, nq_all, metric, far=far)
    n = case.corpus.n
    what = ("sketch", dim, "far" if far else "near", MID[metric])
    tiled = dim == 64
    assert scan_matrix_plan(dim, 8, 12, kp=8)["serves"] == tiled and scan_collect_plan(dim, 8, 12)["serves"] == tiled
    assert scan_masked_plan(dim, 8, 12, sketch_masked=1)["serves"] == tiled
    for k in KS:
        assert tsw.wide_serves(dim, n, k, 0) == tiled and tss.share_serves(dim, n, k, 0) == tiled
    c16, c32 = head(case, 16), head(case, 32)
    settled = 0
    with tsm.open_sketched(dim, metric) as ix:
        ix.load(case.corpus.packed)
        for qi, one in lone_cases(case):   # lone calls: the one-query kernel
            settled += sketch_topk(ix, one, what + ("lone", qi), 1)
        ix.set_option("sketch_matrix", 1)
        settled += sketch_topk(ix, c16, what + ("grouped",), tsm.grouped_passes(16) if tiled else None)
        ix.set_option("sketch_matrix", 0)
        settled += sketch_topk(ix, c16, what + ("matrix",), tsm.matrix_passes(16) if tiled else None)
        ix.set_option("sketch_wide", 2)
        settled += sketch_topk(ix, c32, what + ("wide",), tsw.forced_passes(32) if tiled else None)
        ix.set_option("sketch_wide", 0)
        if dim == 64:
            ix.set_option("sketch_share", 2)
            settled += sketch_topk(ix, case, what + ("shared",), tss.forced_passes(136))
            ix.set_option("sketch_share", 0)
        assert settled > 0 or far, "the sketch settled no query: S and D were never checked"
        # radius searches through the sketch: lone and a batch of 16 with one sweep per query (radius_mq = 0)
        ix.set_option("sketch_radius", 1)
        ix.set_option("radius_mq", 0)
        ix.reset_stats()
        calls = 0
        for kind in range(len(cases.RADIUS_KINDS)):
            for lone in (False, True):
                for recs, _ in radius(ix, c16, kind, what, lone=lone):
                    assert np.isin(recs["pass_"], (_lib.SZG_CERT_SKETCH_RADIUS, _lib.SZG_CERT_RADIUS_SINGLE)).all(), recs["pass_"]
                    calls += len(recs)
        st = ix.stats()
        assert st["sketch_radius_queries"] + st["sketch_radius_fallbacks"] == calls, (what, st)
        assert st["sketch_radius_queries"] > 0 or far, (what, st)
        # the masked forms: one shared resident mask, then tombstones
        ix.set_option("sketch_masked", 1)
        allow = case.keep_mask()
        with ix.mask(allow) as m:
            sketch_topk(ix, c16, what + ("one mask",), tsm.matrix_passes(16) if tiled else None, eligible=allow, masks=m)
            info = ix.sketch_masked_info()
            assert (info["launches"] >= 1) == tiled and info["skip_launches"] == info["launches"], (what, info)
            for qi, one in lone_cases(case):
                sketch_topk(ix, one, what + ("one mask", "lone", qi), 1, eligible=allow, masks=m)
            for kind in range(len(cases.RADIUS_KINDS)):
                radius(ix, c16, kind, what + ("one mask",), eligible=allow, masks=m)
                radius(ix, c16, kind, what + ("one mask",), eligible=allow, lone=True, masks=m)
        dead = np.zeros(n, dtype=bool)
        dead[case.copies[1]] = True
        assert ix.tombstone_rows(np.flatnonzero(dead)) == 1
        sketch_topk(ix, c16, what + ("tombstone",), tsm.matrix_passes(16) if tiled else None, eligible=~dead)
        assert (ix.sketch_masked_info()["launches"] >= 1) == tiled
        for qi, one in lone_cases(case):
            sketch_topk(ix, one, what + ("tombstone", "lone", qi), 1, eligible=~dead)
        for kind in range(len(cases.RADIUS_KINDS)):
            radius(ix, c16, kind, what + ("tombstone",), eligible=~dead)
            radius(ix, c16, kind, what + ("tombstone",), eligible=~dead, lone=True)


# ---- cosine: queries parallel to a row ------------------------------------------------------------------------------------------

PARALLEL = [(32, 40, 0), (32, 40, 1), (16, 17, 1), (8, 100, 1), (64, 24, 0)]


@pytest.mark.parametrize("bits,dim,mq", PARALLEL, ids=["%db-d%d-mq%d" % c for c in PARALLEL])
def test_cosine_parallel_queries(bits, dim, mq):
    """Q = c decode(r), c in (1, 0.5, 3), and a query a few spacings off parallel, for a row below index k and one above
    it: the reference's unclamped acos gives 0 or NaN there, and a NaN among the first k rows sends the query to the
    replay.  The answers -- rows, float64 distances bit for bit, NaN where the oracle has NaN -- and K / L on what is
    recorded (a query the replay answered may leave no bound on its pair: the pair condition is not asked here)."""
    case = cases.build_parallel(bits, dim, 16)
    what = ("parallel", bits, dim, "multi_query", mq)
    with tgc.open_index(case.corpus, sketch=0, multi_query=mq) as ix:
        for k in KS:
            topk(ix, case, k, what, pairs=False)
        for kind in (1, 2, 3, 4):
            radius(ix, case, kind, what, pairs=False)
        dead = np.zeros(case.corpus.n, dtype=bool)
        dead[case.r0] = True
        ix.tombstone_rows(np.flatnonzero(dead))
        for k in KS:
            topk(ix, case, k, what + ("tombstone",), eligible=~dead, pairs=False)


def test_bf16_sweep_query_at_subnormal_spacings_of_zero_rows():
    """A query within a few float32-subnormal spacings of all-zero rows, through the bfloat16 sweep's own keys (the score
    matrix and the radius batch): the float32 key is 0 where the numpy emulation of the operands, which sums in
    float64, has 1e-90.  cert_check.bf16_emulated's tolerance carries float32's range (4 n 2^-126) for this; K holds
    through key_eps' own constant.  (scripts/fuzz_gpu.py found it: seed 21, iterations 873 and 1392.)"""
    dim, nq = 17, 16
    n = cases.n_rows(nq, dim)
    seed = cases.SEED + 990000
    rows = orc.synth_rows(seed, 0, n, dim, 32).copy()
    zero = [9, 12, 700, n - 1]
    rows[zero] = 0
    Q = orc.synth_vectors(seed + 1, 0, nq, dim)
    Q[2] = np.float64(np.float32(1.4e-45)) * np.resize([1.0, -2.0, 3.0], dim)
    case = cases.Case(cc.Corpus(rows, dim, 32, 0), Q, [(2, r, "zero row") for r in zero], (), zero[0])
    assert (case.dists()[2, zero] > 0).all() and (case.dists()[2, zero] < 1e-43).all()
    what = ("zero rows", "bf16")
    with tgc.open_index(case.corpus, sketch=0, contexts=1, force_matrix=1) as ix:
        recs, ents = topk(ix, case, 10, what)
        assert (tgc.first_pass(recs)["keys"] == _lib.SZG_CERT_KEYS_SHARED_BF16).all()
        assert cc.check_bf16_tight(case.corpus, case.Q, recs, ents, MARGINS, what) > 0
        rec = tgc.first_pass(recs)[tgc.first_pass(recs)["query"] == 2][0]
        e = ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]
        assert (e["key"][np.isin(e["row"], zero)] == 0.0).all(), "the float32 key at a zero row is 0"
        for kind in (1, 3):
            (recs, ents), = radius(ix, case, kind, what)
            assert (recs["pass_"] == _lib.SZG_CERT_RADIUS_SHARED).all() and (recs["sweep"] == 2).all()
            assert cc.check_bf16_tight(case.corpus, case.Q, recs, ents, MARGINS, what) > 0
