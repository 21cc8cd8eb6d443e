"""Every sweep's keys and certificates against float64, row by row.

The other GPU tests compare final rows and distances with the oracle.  An answer is exact only because of a chain of
bounds, and a kernel that breaks one -- a dropped piece of a ragged row, a stale operand for
one lane -- almost never changes an answer.  Here the handle's certificate trace (szg_debug_trace_certificates) hands
over what each pass gave to certification, and syzgydb_amd/cert_check.py checks the claims themselves against a plain
float64 / longdouble reference computed from the oracle-decoded rows:

    K  |key - real| <= ub - key for every candidate        L  left-out rows have real >= thr_min
    C  a collect sweep returned every row under its threshold, and nothing above it
    S  the sketch pre-pass's D - slack                     A  the answers are the oracle's

A radius that covers every row (cosine 1, Euclid 1e25: the threshold becomes "take everything") turns the collect form
of each sweep into a dump of that kernel's key for EVERY row, lane position and tile position.  Each family forces its
kernel by options and confirms from the statistics and the records' pass kinds that it served.

The bfloat16 sweeps get a tighter check beside K (whose band, 2^-7, would hide a dropped element): their operand
rounding is emulated in numpy -- cert_check.bf16_emulated says which operand is rounded where -- and the recorded key
must lie within the float32-accumulation part of key_eps's bfloat16 branch of the emulated key.

Which kernel of a family served: the statistics and the records tell the sweep kind (one-sweep, int8, bfloat16) and
the form of its tail; which kernel of the kind ran -- mq_score_i8s or mq_score_i8, the staged or a direct bfloat16
kernel -- is not reported by the library and is INFERRED here from the launchers' rules (kernels_mq_i8.hip
launch_mq_score_i8_m: rows of 3, 6 or 12 whole 64-byte steps with resident norms take the shaped kernel; kernels_mq.hip
launch_mq_score_bf16: 16-bit rows with resident norms and tiled 8-bit rows take the direct kernels, the rest the
staged one).  A change to those rules has to move the dimensions chosen below with it.

Rows per shared sweep: its grid is one block per compute unit, a block's waves take 16-row tiles round robin, so with
W <= 12 waves per block  n = 16 (256 * 12 + 12 + 1) - 11 = 49 349  rows give at least two blocks at least two tiles per wave and
a last tile of 5 rows (kernels of fewer waves walk more tiles each).

MARGINS keeps the largest |key - real| / eps per pass kind, width and metric (scripts/dev_certificates.py runs this
file, checks that every pass kind and arithmetic left a margin, and writes them to profiles/certificate_margins.txt).
"""
import functools
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as orc
import scan_lattice as lat
from syzgydb_amd import ScanIndex, _lib
from syzgydb_amd import cert_check as cc

pytestmark = pytest.mark.gpu

SEED = 0x53595A4700002000
METRICS = (0, 1)   # Euclidean, cosine
METRIC_IDS = {0: "euc", 1: "cos"}
MARGINS = cc.Margins()
POOL = ThreadPoolExecutor(8)   # the oracle's C calls release the interpreter lock
ALL_ROWS = {0: 1.0e25, 1: 1.0}   # a radius that takes every row
GROUP_K = 43   # the largest k whose lists stay in registers (kp = 64): grouped launches still form


CUS = 256   # compute units of an MI355X (a card with fewer only gives every wave more tiles)


def shared_rows():
    return 16 * (CUS * 12 + 12 + 1) - 11


@functools.lru_cache(maxsize=2)
def synth_corpus(seed, n, dim, bits):
    cuts = np.linspace(0, n, 9).astype(np.int64)
    parts = POOL.map(lambda i: orc.synth_rows(seed, int(cuts[i]), int(cuts[i + 1] - cuts[i]), dim, bits), range(8))
    c = cc.Corpus(np.concatenate(list(parts)), dim, bits, 0)
    c.check_decode(orc)
    return c


def open_index(corpus, seed=None, rows=None, **options):
    ix = ScanIndex(corpus.dim, corpus.bits, corpus.metric)
    if seed is not None:
        ix.synth(corpus.n, seed)
        at = corpus.n - 1
        assert (ix.read_rows(at, 1) == corpus.packed[at:]).all()   # device synthesis == the oracle's
    else:
        ix.load(corpus.packed if rows is None else rows)
    for name, value in options.items():
        ix.set_option(name, value)
    ix.trace_certificates(True)
    return ix


def assert_same(got_rows, got_dist, want, what):
    want_rows, want_dist = want
    assert [int(x) for x in got_rows] == [int(x) for x in want_rows], ("rows differ", what)
    g, w = np.asarray(got_dist, dtype=np.float64), np.asarray(want_dist, dtype=np.float64)
    assert ((g == w) | (np.isnan(g) & np.isnan(w))).all(), ("distances not bit-equal", what, g, w)


def traced_topk(ix, corpus, Q, k, what, eligible=None, skips=0, **filt):
    """One top-k call: K, L (and C, S) on its records, A on its answers.  -> (summary, records, entries)"""
    Q = np.atleast_2d(Q)
    r, d, cnt = ix.search_topk(Q, k, **filt)
    recs, ents, dropped = ix.certificates()
    dists = sketch = None
    if (recs["pass_"] == _lib.SZG_CERT_SKETCH).any():
        dists = np.stack(list(POOL.map(lambda q: orc.all_distances(corpus.packed, corpus.dim, corpus.bits, corpus.metric, q), Q)))
        info = ix.sketch_info()
        if info["exists"] and info["in_sync"]:   # the sketch sweep's own keys and lists too (K_s, L_s, D)
            sketch = (cc.Corpus(ix.sketch_rows()[0], corpus.dim, 8, corpus.metric), info["gscale"], info["exc_rows"])
    s = cc.check(corpus, Q, recs, ents, dropped, eligible=eligible, dists=dists, margins=MARGINS, what=what + ("k", k),
                 sketch=sketch)
    assert s.skipped <= skips, ("candidates without a bound on a corpus that plants none", what, s.skipped, sorted(s.skipped_rows)[:8])
    first = recs[(recs["pass_"] == _lib.SZG_CERT_TOPK) | (recs["pass_"] == _lib.SZG_CERT_SKETCH)]
    settled = first[(first["pass_"] == _lib.SZG_CERT_TOPK) | (first["certified"] == 1)]
    assert sorted(int(x) for x in settled["query"]) == list(range(Q.shape[0])), ("one first-pass record per query", what)
    el = None if eligible is None else np.broadcast_to(eligible, (Q.shape[0], corpus.n))
    todo = range(Q.shape[0])
    want = POOL.map(lambda qi: orc.search_exact(corpus.packed, corpus.dim, corpus.bits, corpus.metric, Q[qi], k=k,
                                                allow=None if el is None else el[qi].astype(np.uint8))[:2], todo)
    for qi, w in zip(todo, want):
        assert_same(r[qi, : cnt[qi]], d[qi, : cnt[qi]], w, what + ("k", k, "query", qi))
    return s, recs, ents


def traced_radius_all(ix, corpus, Q, what, eligible=None, skips=0, shared=None, **filt):
    """One radius batch that takes every row: K for every (query, row), C = every eligible row is a hit."""
    Q = np.atleast_2d(Q)
    radii = [ALL_ROWS[corpus.metric]] * Q.shape[0]
    room = Q.shape[0] * corpus.n   # (a batch that does not fit the caller's buffer is searched twice: two sets of records)
    if shared:   # the first batch on a context finds buffers of 1024 hits per query and sweeps each query again on its
        ix.trace_certificates(False)   # own; the next one has room (RadiusCall::finish)
        ix.search_radius_batch(Q, radii, capacity=room, **filt)
        ix.trace_certificates(True)
    hits = ix.search_radius_batch(Q, radii, capacity=room, **filt)
    recs, ents, dropped = ix.certificates()
    s = cc.check(corpus, Q, recs, ents, dropped, eligible=eligible, margins=MARGINS, what=what + ("radius",))
    assert s.skipped <= skips, ("candidates without a bound on a corpus that plants none", what, s.skipped)
    assert sorted(int(x) for x in recs["query"]) == list(range(Q.shape[0])), ("one collect record per query", what)
    if shared is not None:
        want = _lib.SZG_CERT_RADIUS_SHARED if shared else _lib.SZG_CERT_RADIUS_SINGLE
        assert (recs["pass_"] == want).all() and (recs["thr"] >= cc.TAKE_ALL).all(), (what, recs["pass_"], recs["thr"])
        if shared:
            assert (recs["sweep"] == shared).all(), (what, recs["sweep"])
    el = np.broadcast_to(np.ones(corpus.n, dtype=bool) if eligible is None else eligible, (Q.shape[0], corpus.n))
    for qi in range(Q.shape[0]):
        assert len(hits[qi][0]) <= int(el[qi].sum())
        if skips == 0 and corpus.finite.all():
            assert len(hits[qi][0]) == int(el[qi].sum()), (what, "query", qi)
    return s, recs, ents


def first_pass(recs):
    """The records of the first top-k passes (a query that is not certified adds an escalation record behind its own)."""
    return recs[recs["pass_"] == _lib.SZG_CERT_TOPK]


def keys_by_row(recs, ents, qi):
    rec = first_pass(recs)[first_pass(recs)["query"] == qi][0]
    e = ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]
    order = np.argsort(e["row"], kind="stable")
    return e["row"][order], e["key"][order].view(np.uint32)


# ---- the one-sweep kernel over its lattice ------------------------------------------------------------------------------

CELLS = lat.all_cells()
CELL_METRIC = [(c, m) for c in CELLS for m in METRICS]
CELL_METRIC_IDS = ["%s-%s" % (lat.cell_id(c), METRIC_IDS[m]) for c, m in CELL_METRIC]


def cell_seed(c):
    return SEED + c.bits * 100000 + c.r16 * 16


def assert_scan_kernel_served(ix):
    st = ix.stats()
    assert st["mq_queries"] == 0 and st["sketch_queries"] == 0 and st["scan_launches"] > 0, st


@pytest.mark.parametrize("cell,metric", CELL_METRIC, ids=CELL_METRIC_IDS)
def test_scan_kernel_small_rows(cell, metric):
    """Every cell of the lattice at its small row count, three queries per call: top-k with register lists (k = 10) and
    LDS lists (k = 80), and the all-rows radius batch -- K for every row of the corpus, at every lane position of the
    cell's map.  Then the same under a filter mask, and with tombstones: L and C count eligible rows only.  8-bit cells
    also with scan_group 2 and 4 and scan_norms 0 and 1 at k = 43 (kp = 64, the longest lists a grouped launch keeps): the
    recorded keys of all 64 candidates per query are bit-equal to those of group 1."""
    seed = cell_seed(cell)
    corpus = synth_corpus(seed, cell.small_n, cell.dim, cell.bits).with_metric(metric)
    n = corpus.n
    Q = orc.synth_vectors(seed + 1, 0, 3, cell.dim)
    what = (lat.cell_id(cell), METRIC_IDS[metric])
    rng = np.random.default_rng(seed & 0xFFFFFFFF)
    allow = rng.random(n) < 0.6
    dead = np.arange(n) % 7 == 3
    with open_index(corpus, seed, multi_query=0, sketch=0, scan_group=1) as ix:
        _, recs10, ents10 = traced_topk(ix, corpus, Q, 10, what)
        assert (first_pass(recs10)["keys"] == _lib.SZG_CERT_KEYS_SINGLE).all() and (recs10["sweep"] == 0).all()
        traced_topk(ix, corpus, Q, 80, what)
        s, _, _ = traced_radius_all(ix, corpus, Q, what, shared=0)
        assert s.checked == 3 * n
        if cell.bits == 8:
            # (collect sweeps never form groups, so there is no all-rows dump of the grouped kernels: the longest lists
            # that still form groups, 64 candidates per query, are compared entry by entry)
            assert lat.kp_of(GROUP_K) <= 64 < lat.kp_of(GROUP_K + 1)
            _, recs1, ents1 = traced_topk(ix, corpus, Q, GROUP_K, what + ("scan_group", 1))
            for group, norms in ((2, 0), (4, 0), (2, 1), (4, 1)):
                ix.set_option("scan_group", group)
                ix.set_option("scan_norms", norms)
                _, recs, ents = traced_topk(ix, corpus, Q, GROUP_K, what + ("scan_group", group, "scan_norms", norms))
                for qi in range(3):
                    r1, k1 = keys_by_row(recs1, ents1, qi)
                    rg, kg = keys_by_row(recs, ents, qi)
                    assert (r1 == rg).all() and (k1 == kg).all(), ("grouped keys differ from group 1", what, group, norms, qi)
            ix.set_option("scan_group", 1)
        traced_topk(ix, corpus, Q, 10, what + ("allow 0.6",), eligible=allow, allow=np.stack([allow] * 3))
        traced_radius_all(ix, corpus, Q, what + ("allow 0.6",), eligible=allow, allow=np.stack([allow] * 3))
        ix.tombstone_rows(np.flatnonzero(dead))
        traced_topk(ix, corpus, Q, 10, what + ("tombstones",), eligible=~dead)
        traced_radius_all(ix, corpus, Q, what + ("tombstones",), eligible=~dead)
        assert_scan_kernel_served(ix)


def deep_cells():
    out = []
    for bits in lat.WIDTHS:
        cs = lat.cells(bits)
        out += [c for c in cs if c.kind == "shape"]
        for want in ("dense", "ragged"):
            out.append(min((c for c in cs if c.kind == "class" and c.cls[3] == want), key=lambda c: c.deep_n * c.dim))
    return out


DEEP = [(c, m) for c in deep_cells() for m in METRICS]


@pytest.mark.parametrize("cell,metric", DEEP, ids=["%s-%s" % (lat.cell_id(c), METRIC_IDS[m]) for c, m in DEEP])
def test_scan_kernel_deep_rows(cell, metric):
    """The all-rows radius search at the deep row count, where every wave walks several rows in the predicate-free
    dense phase: K for every row.  The row-shape-specialised kernels, and per width the cheapest dense and ragged class."""
    seed = cell_seed(cell) + 7
    corpus = synth_corpus(seed, cell.deep_n, cell.dim, cell.bits).with_metric(metric)
    q = orc.synth_vectors(seed + 1, 0, 1, cell.dim)
    with open_index(corpus, seed, multi_query=0, sketch=0) as ix:
        s, recs, _ = traced_radius_all(ix, corpus, q, (lat.cell_id(cell), METRIC_IDS[metric], "deep"))
        assert s.checked == corpus.n and (recs["pass_"] == _lib.SZG_CERT_RADIUS_SINGLE).all()
        assert_scan_kernel_served(ix)


# ---- the shared sweeps ----------------------------------------------------------------------------------------------------

def shared_case(bits, dim, nq, metric, seed_off=0):
    seed = SEED + 5000 + bits * 1000 + dim + seed_off
    corpus = synth_corpus(seed, shared_rows(), dim, bits).with_metric(metric)
    return seed, corpus, orc.synth_vectors(seed + 1, 0, nq, dim)


def masked_and_tombstoned(ix, corpus, Q, what, shared, tight=False):
    """One masked and one tombstoned pass of a shared-sweep family: a resident mask shared by every query, then
    tombstones; top-k and all-rows radius each."""
    n = corpus.n
    rng = np.random.default_rng(n + corpus.dim)
    allow = rng.random(n) < 0.7
    dead = np.zeros(n, dtype=bool)
    dead[rng.integers(0, n, 300)] = True
    dead[n - 1] = True   # (in the partial last tile)
    with ix.mask(allow) as m:
        traced_topk(ix, corpus, Q, 10, what + ("resident mask",), eligible=allow, masks=m)
        _, recs, ents = traced_radius_all(ix, corpus, Q, what + ("resident mask",), eligible=allow, shared=shared, masks=m)
    ix.tombstone_rows(np.flatnonzero(dead))
    traced_topk(ix, corpus, Q, 10, what + ("tombstones",), eligible=~dead)
    _, recs, ents = traced_radius_all(ix, corpus, Q, what + ("tombstones",), eligible=~dead, shared=shared)
    if tight:
        assert cc.check_bf16_tight(corpus, Q, recs, ents, MARGINS, what) > 0


I8_CASES = [(bits, dim, nq, m) for bits, dims in ((8, (768, 384, 192, 100)), (4, (1536, 768, 384, 200)))
            for dim in dims for nq in (16, 48) for m in METRICS]


@pytest.mark.parametrize("bits,dim,nq,metric", I8_CASES, ids=["%db-d%d-q%d-%s" % (b, d, q, METRIC_IDS[m]) for b, d, q, m in I8_CASES])
def test_int8_shared_sweep(bits, dim, nq, metric):
    """mq_score_i8s_kernel (rows of 12, 6 and 3 whole 64-byte steps) and mq_score_i8_kernel (a ragged row that ends in
    a short step), 16 and 48 queries per sweep: top-k (SharedInt8 lists) and the all-rows radius batch (the collect
    form: the sweep's exact integer key of every row against the integer bound)."""
    seed, corpus, Q = shared_case(bits, dim, nq, metric)
    what = ("int8", bits, dim, nq, METRIC_IDS[metric])
    with open_index(corpus, seed, sketch=0, contexts=1) as ix:
        _, recs, _ = traced_topk(ix, corpus, Q, 10, what)
        first = first_pass(recs)
        assert (first["keys"] == _lib.SZG_CERT_KEYS_SHARED_INT8).all() and (first["sweep"] == 1).all(), (first["keys"], first["sweep"])
        s, _, _ = traced_radius_all(ix, corpus, Q, what, shared=1)
        assert s.checked == nq * corpus.n
        st = ix.stats()
        assert st["mq_queries"] == 3 * nq and st["mq_bf16_sweeps"] == 0, st   # (top-k, and the radius batch twice)
        if nq == 16 and dim in (768, 100, 1536, 200):
            masked_and_tombstoned(ix, corpus, Q, what, 1)


def bf16_forms(ix, corpus, Q, what, tight_radius=True):
    """The three tails of a bfloat16 shared sweep -- fused with the refine launch (Bf16Band), fused with separate
    re-score and select launches (Bf16Rescored), the score matrix (SharedBf16, the sweep's own keys: the tight check
    applies) -- then the all-rows radius batch (the sweep's own key of every row: K and the tight check)."""
    seen = set()
    for options, want in (({}, _lib.SZG_CERT_KEYS_BF16_BAND), ({"force_no_refine": 1}, _lib.SZG_CERT_KEYS_BF16_RESCORED),
                          ({"force_matrix": 1}, _lib.SZG_CERT_KEYS_SHARED_BF16)):
        for name, value in options.items():
            ix.set_option(name, value)
        _, recs, ents = traced_topk(ix, corpus, Q, 10, what + (cc.KEYS_NAMES[want],))
        # (a batch whose error band holds more candidates than the refine launch takes is redone through the score
        # matrix: in three dimensions that happens, and the lists then hold the sweep's own keys)
        first = first_pass(recs)
        kinds = set(int(x) for x in first["keys"])
        assert kinds <= {want, _lib.SZG_CERT_KEYS_SHARED_BF16} and (first["sweep"] == 2).all(), (what, first["keys"], first["sweep"])
        if corpus.dim >= 17:
            assert kinds == {want}, (what, kinds, ix.stats())
        band = first[first["keys"] != _lib.SZG_CERT_KEYS_SHARED_BF16]
        assert np.isfinite(band["thr_min"]).all()   # L held for the threshold (and the band's edge): they entered thr_min
        if _lib.SZG_CERT_KEYS_SHARED_BF16 in kinds:
            assert cc.check_bf16_tight(corpus, Q, recs, ents, MARGINS, what) > 0
        seen |= kinds
        for name in options:
            ix.set_option(name, 0)
    s, recs, ents = traced_radius_all(ix, corpus, Q, what, shared=2)
    assert s.checked == Q.shape[0] * corpus.n
    assert cc.check_bf16_tight(corpus, Q, recs, ents, MARGINS, what) == Q.shape[0] * corpus.n
    st = ix.stats()
    assert st["mq_bf16_sweeps"] >= 5 and st["mq_queries"] >= 5 * Q.shape[0], st
    assert len(seen) == 3 or corpus.dim < 17, (what, seen)
    return seen


BF16S_CASES = [(bits, dim, nq, m) for bits, dims in ((32, (3, 17, 40, 768)), (64, (3, 17, 24, 768)))
               for dim in dims for nq in (16, 96) for m in METRICS]


@pytest.mark.parametrize("bits,dim,nq,metric", BF16S_CASES, ids=["%db-d%d-q%d-%s" % (b, d, q, METRIC_IDS[m]) for b, d, q, m in BF16S_CASES])
def test_bf16_staged_sweep(bits, dim, nq, metric):
    """mq_score_bf16s_kernel on 32- and 64-bit rows: dimensions 3 and 17 (a lone short step), one whole 128-byte step
    plus a short one (40 floats, 24 doubles: also an odd number of half K-steps) and 768."""
    seed, corpus, Q = shared_case(bits, dim, nq, metric)
    what = ("bf16s", bits, dim, nq, METRIC_IDS[metric])
    with open_index(corpus, seed, sketch=0, contexts=1) as ix:
        bf16_forms(ix, corpus, Q, what)
        if nq == 16 and dim in (17, 768):
            masked_and_tombstoned(ix, corpus, Q, what, 2, tight=True)


BF16D_CASES = [(16, dim, nq, m) for dim in (3, 17, 40, 72, 768) for nq in (16, 96) for m in METRICS] + \
              [(8, dim, 96, m) for dim in (64, 192, 320, 768) for m in METRICS]


@pytest.mark.parametrize("bits,dim,nq,metric", BF16D_CASES, ids=["%db-d%d-q%d-%s" % (b, d, q, METRIC_IDS[m]) for b, d, q, m in BF16D_CASES])
def test_bf16_direct_sweeps(bits, dim, nq, metric):
    """mq_score_bf16d_kernel (16-bit rows, resident norms: 3, 17, 40 and 72 elements -- one and two 64-byte K-steps
    plus a short one, an odd number of double steps -- and 768) and mq_score_bf16d8_kernel (8-bit rows in whole
    64-byte steps, 96 queries: 1, 3, 5 and 12 steps).  The row count leaves a partial last tile.  8-bit radius batches
    stay on the int8 sweep (a radius is the threshold), so the 8-bit kernel's own keys are checked through its
    SharedBf16 lists."""
    seed, corpus, Q = shared_case(bits, dim, nq, metric, seed_off=77)
    what = ("bf16d", bits, dim, nq, METRIC_IDS[metric])
    with open_index(corpus, seed, sketch=0, contexts=1) as ix:
        if bits == 16:
            bf16_forms(ix, corpus, Q, what)
            if nq == 16 and dim in (17, 768):
                masked_and_tombstoned(ix, corpus, Q, what, 2, tight=True)
            return
        for options, want in (({}, _lib.SZG_CERT_KEYS_BF16_BAND), ({"force_no_refine": 1}, _lib.SZG_CERT_KEYS_BF16_RESCORED),
                              ({"force_matrix": 1}, _lib.SZG_CERT_KEYS_SHARED_BF16)):
            for name, value in options.items():
                ix.set_option(name, value)
            _, recs, ents = traced_topk(ix, corpus, Q, 10, what + (cc.KEYS_NAMES[want],))
            first = first_pass(recs)
            assert (first["keys"] == want).all() and (first["sweep"] == 2).all(), (what, first["keys"], first["sweep"])
            if want == _lib.SZG_CERT_KEYS_SHARED_BF16:
                assert cc.check_bf16_tight(corpus, Q, recs, ents, MARGINS, what) > 0
            for name in options:
                ix.set_option(name, 0)
        st = ix.stats()
        assert st["mq_bf16_sweeps"] == 3 and st["mq_queries"] == 3 * nq, st
        if dim == 192:
            n = corpus.n
            dead = np.arange(n) % 11 == 5
            allow = np.arange(n) % 3 != 1
            traced_topk(ix, corpus, Q, 10, what + ("allow",), eligible=allow, allow=np.stack([allow] * nq))
            ix.tombstone_rows(np.flatnonzero(dead))
            traced_topk(ix, corpus, Q, 10, what + ("tombstones",), eligible=~dead)


def child_staged16(dim):
    """Runs in a child process with SZG_NO_ROW_NORMS set: 16-bit rows then take mq_score_bf16s_kernel (no resident norms)."""
    assert os.environ.get("SZG_NO_ROW_NORMS")
    for metric in METRICS:
        seed, corpus, Q = shared_case(16, dim, 16, metric, seed_off=33)
        with open_index(corpus, seed, sketch=0, contexts=1) as ix:
            bf16_forms(ix, corpus, Q, ("bf16s", 16, dim, 16, METRIC_IDS[metric]))
    for what, ratio in MARGINS.worst.items():   # handed to the parent, which keeps the margins of the whole run
        print("MARGIN\t%s" % json.dumps([list(what), ratio, MARGINS.count[what]]))


@pytest.mark.parametrize("dim", (3, 17, 40, 768))
def test_bf16_staged_sweep_16bit_without_resident_norms(dim):
    """16-bit rows through the staged kernel: SZG_NO_ROW_NORMS is read once per process, so the cases run in a child."""
    env = dict(os.environ, SZG_NO_ROW_NORMS="1")
    code = "import sys; sys.path[:0] = %r; import test_gpu_certificates as t; t.child_staged16(%d)" % (
        [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))], dim)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-4000:], p.stderr[-4000:])
    got = [json.loads(line.split("\t", 1)[1]) for line in p.stdout.splitlines() if line.startswith("MARGIN\t")]
    assert got, p.stdout[-2000:]
    for what, ratio, count in got:
        assert ratio <= 1.0, (what, ratio)
        what[2] += "/no-norms"   # (16-bit rows through the staged kernel: kept apart from the direct kernel's margins)
        MARGINS.note(tuple(what), ratio, count)


# ---- the sketch pre-pass ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS, ids=["euc", "cos"])
def test_sketch_certificate(metric):
    """float32 rows through the 8-bit sketch pre-pass (sketch = 1, sketch_min_rows lowered), sketch_list automatic and
    >= kp, sketch_planes 0 and 3: S for every query the sketch settled -- every eligible row outside its candidates is at
    oracle distance >= D - slack.  Then rows are appended and overwritten (slack and the Euclidean scale move) and a
    mask and tombstones come in.  Queries it hands over are checked as first top-k passes of the full sweep."""
    dim, n0, n1 = 96, 5000, 6000
    seed = SEED + 9000 + metric
    vec = orc.synth_vectors(seed, 0, n1, dim)
    Q = orc.synth_vectors(seed + 1, 0, 12, dim) * 0.7
    settled = 0
    with ScanIndex(dim, 32, metric) as ix:
        ix.load(orc.encode_rows(vec[:n0], 32))
        for name, value in (("sketch", 1), ("sketch_min_rows", 1000), ("multi_query", 0)):
            ix.set_option(name, value)
        ix.trace_certificates(True)
        corpus = cc.Corpus(orc.encode_rows(vec[:n0], 32), dim, 32, metric)
        for lst, planes in ((0, 0), (100, 0), (0, 3)):
            ix.set_option("sketch_list", lst)
            ix.set_option("sketch_planes", planes)
            s, recs, _ = traced_topk(ix, corpus, Q, 10, ("sketch", METRIC_IDS[metric], "list", lst, "planes", planes))
            sk = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]
            assert len(sk) == 12 and np.isfinite(sk["slack"]).all()
            settled += int((sk["certified"] == 1).sum())
        # appended rows twice as long (the Euclidean scale moves: a rebuild), overwritten rows, then a filter
        vec[n0:] *= 2.0
        ix.append(orc.encode_rows(vec[n0:], 32))
        vec[17] = vec[17] * -0.5
        vec[4000] = vec[3] * 1.25
        for r in (17, 4000):
            ix.overwrite(r, orc.encode_rows(vec[r:r + 1], 32))
        corpus = cc.Corpus(orc.encode_rows(vec, 32), dim, 32, metric)
        assert settled > 0, "the sketch settled no query of the plain corpus: S was never checked"
        before = settled
        s, recs, _ = traced_topk(ix, corpus, Q, 10, ("sketch", METRIC_IDS[metric], "after appends"))
        settled += int(((recs["pass_"] == _lib.SZG_CERT_SKETCH) & (recs["certified"] == 1)).sum())
        allow = np.arange(n1) % 5 != 2
        s, recs, _ = traced_topk(ix, corpus, Q, 10, ("sketch", METRIC_IDS[metric], "allow"), eligible=allow, allow=np.stack([allow] * 12))
        settled += int(((recs["pass_"] == _lib.SZG_CERT_SKETCH) & (recs["certified"] == 1)).sum())
        ix.tombstone_rows(np.arange(0, n1, 9))
        el = np.arange(n1) % 9 != 0
        s, recs, _ = traced_topk(ix, corpus, Q, 10, ("sketch", METRIC_IDS[metric], "tombstones"), eligible=el)
        settled += int(((recs["pass_"] == _lib.SZG_CERT_SKETCH) & (recs["certified"] == 1)).sum())
        st = ix.stats()
        assert st["sketch_queries"] == settled and settled > before, (st, settled, before)


# ---- escalation ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", lat.WIDTHS)
def test_forced_escalation(bits):
    """force_escalate on one case per row width, a shared-sweep batch and one sweep per query: the escalation's collect
    record satisfies C and K against the single-query bound, and every reference answer is inside it."""
    dim, n, k = {4: 200, 8: 100, 16: 72, 32: 40, 64: 24}[bits], 6000, 10
    seed = SEED + 12000 + bits
    base = synth_corpus(seed, n, dim, bits)
    Q = orc.synth_vectors(seed + 1, 0, 16, dim)
    for metric in METRICS:
        corpus = base.with_metric(metric)
        for mq in (1, 0):
            with open_index(corpus, seed, sketch=0, multi_query=mq, force_escalate=1) as ix:
                what = ("escalation", bits, METRIC_IDS[metric], "multi_query", mq)
                s, recs, ents = traced_topk(ix, corpus, Q, k, what)
                esc = recs[recs["pass_"] == _lib.SZG_CERT_ESCALATION]
                assert len(esc) == 16 and (esc["sweep"] == 0).all() and ix.stats()["escalations"] == 16
                assert ((recs["pass_"] == _lib.SZG_CERT_TOPK) & (recs["certified"] == 0)).sum() == 16
                for rec in esc:
                    qi = int(rec["query"])
                    rows = set(int(x) for x in ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]["row"])
                    want = orc.search_exact(corpus.packed, dim, bits, metric, Q[qi], k=k)[0]
                    assert set(int(x) for x in want) <= rows, ("a reference answer outside the escalation's hits", what, qi)


# ---- adversarial values ---------------------------------------------------------------------------------------------------------

def loaded(vec, bits, metric, **options):
    rows = orc.encode_rows(vec, bits)
    corpus = cc.Corpus(rows, vec.shape[1], bits, metric)
    return corpus, open_index(corpus, **options)


@pytest.mark.parametrize("dim", (1, 2, 3, 16))
def test_adversarial_few_dims_far_from_origin(dim):
    """The corpus of test_bf16_sweep_few_dims_far_from_origin (every row and query within a few degrees of one
    direction: bfloat16 roundings that all point the same way) under K and L, fused and matrix form,
    and the sweep's own keys under the tight check."""
    n = 5000
    rng = np.random.default_rng(7000 + 10 * dim)
    vec = rng.uniform(-1, 1, (n, dim)) * 1e3 + 5e3
    Q = rng.uniform(-1, 1, (16, dim)) * 1e3 + 5e3
    for metric in METRICS:
        corpus, ix = loaded(vec, 32, metric, sketch=0)
        with ix:
            for matrix in (0, 1):
                ix.set_option("force_matrix", matrix)
                _, recs, ents = traced_topk(ix, corpus, Q, 10, ("far from origin", dim, METRIC_IDS[metric], matrix))
                assert (first_pass(recs)["sweep"] == 2).all()
                cc.check_bf16_tight(corpus, Q, recs, ents, MARGINS)
            ix.set_option("multi_query", 0)
            traced_topk(ix, corpus, Q[:3], 10, ("far from origin", dim, METRIC_IDS[metric], "one sweep"))


@pytest.mark.parametrize("bits", (32, 64))
def test_adversarial_scales_and_equal_rows(bits):
    """Rows scaled by 1e+18 and 1e-18 (norms near the ends of the float32 range; on 32-bit Euclidean rows the large
    ones overflow the float32 key: those candidates are the planted ones that may be skipped), all-equal rows, and a
    zero cosine query (no bound is claimed: only the answers and the record's shape are checked)."""
    rng = np.random.default_rng(99 + bits)
    dim, n = 48, 4000
    vec = rng.standard_normal((n, dim))
    big, small = np.arange(100, 140), np.arange(200, 240)
    vec[big] *= 1e18
    vec[small] *= 1e-18
    vec[300:400] = vec[300]
    Q = np.concatenate([rng.standard_normal((14, dim)), vec[[100, 200]] * 1.5])
    for metric in METRICS:
        for mq in (1, 0):
            corpus, ix = loaded(vec, bits, metric, sketch=0, multi_query=mq)
            with ix:
                what = ("scales", bits, METRIC_IDS[metric], "multi_query", mq)
                planted = 16 * len(big)
                s, _, _ = traced_topk(ix, corpus, Q, 10, what, skips=planted)
                assert s.skipped_rows <= set(int(x) for x in big), (what, sorted(s.skipped_rows)[:8])
                s, _, _ = traced_radius_all(ix, corpus, Q, what, skips=planted)
                assert s.skipped_rows <= set(int(x) for x in big), (what, sorted(s.skipped_rows)[:8])
    corpus, ix = loaded(vec, bits, 1, sketch=0)
    with ix:
        zero = np.zeros((2, dim))
        zero[1] = Q[0]
        s, recs, _ = traced_topk(ix, corpus, zero, 10, ("zero query", bits), skips=16 * n)
        assert len(recs[recs["pass_"] == _lib.SZG_CERT_TOPK]) == 2


@pytest.mark.parametrize("bits", (4, 8))
def test_adversarial_integer_queries(bits):
    """Queries whose largest element is quantized to the largest magnitude the integer paths accept (|Q| = kMqQmax on
    the shared sweep, 10^6 / kQmax4 on the one-sweep kernel -- the largest element of ANY query is) with every other
    element at the far end of its sign or half a step from a code, on rows that are all-equal, all-0 and all-maxInt."""
    rng = np.random.default_rng(1234 + bits)
    dim, n = {8: 100, 4: 200}[bits], 5000
    vec = rng.uniform(-1, 1, (n, dim))
    vec[10:60] = vec[10]
    vec[60:80] = -1.0
    vec[80:100] = 1.0
    Q = np.sign(rng.standard_normal((16, dim)))
    Q[4:8] *= rng.integers(1, 3, (4, dim)) / 2.0           # +-1 and +-1/2
    Q[8:12] = rng.integers(-32000, 32001, (4, dim)) / 32000.0 + 0.5 / 16000.0   # half a two-plane step off
    Q[12:] = 0.0
    Q[12:, 0] = 1.0                                          # one element carries everything
    Q[13, 1:] = 1.0 / 31999.0
    for metric in METRICS:
        for mq in (1, 0):
            corpus, ix = loaded(vec, bits, metric, sketch=0, multi_query=mq)
            with ix:
                what = ("integer queries", bits, METRIC_IDS[metric], "multi_query", mq)
                _, recs, _ = traced_topk(ix, corpus, Q, 10, what)
                assert (recs[recs["pass_"] == _lib.SZG_CERT_TOPK]["sweep"] == mq).all()
                traced_radius_all(ix, corpus, Q, what)
