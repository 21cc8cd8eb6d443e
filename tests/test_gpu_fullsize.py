"""BASELINE.json's configurations at (or near) full size, checked through
size-independent properties plus oracle spot checks on the rows returned:

  * the returned distances equal the oracle's distance for exactly those rows
    (rows are read back from the device mirror, so this pins decode + distance);
  * results ascend; top-10 is a prefix of top-100 (selection is consistent in k);
  * a radius search at the k-th distance returns the same first k rows;
  * a query equal to a stored row finds that row first;
  * nothing outside the result beats the k-th distance, checked on a random sample
    of rows (any miss of the scan would show up here with probability ~ sample/n).
"""
import numpy as np
import pytest

import oracle as orc
import scan_lattice as lat
from syzgydb_amd import ScanIndex, scan_plan
from syzgydb_amd.synth import synth_vectors

pytestmark = pytest.mark.gpu

CONFIGS = [
    # name, rows, dim, bits, metric, k
    ("cfg1-plumbing", 10_000, 128, 32, 1, 10),
    ("cfg2", 1_000_000, 384, 32, 1, 10),
    ("cfg3", 1_000_000, 768, 8, 1, 10),
    ("headline", 1_000_000, 768, 32, 1, 10),
    ("cfg4-one-gpu-shard", 1_250_000, 768, 32, 0, 100),     # 10M / 8 GPUs
    ("cfg5-slice", 4_000_000, 384, 4, 1, 10),                # 100M x 384 4-bit, a 768 MB slice
    # the two 8-GPU configurations in full on ONE card (30.7 GB and 19.2 GB of 288 GB HBM)
    ("cfg4-full", 10_000_000, 768, 32, 0, 100),
    ("cfg5-full", 100_000_000, 384, 4, 1, 10),
]


def oracle_dist_for(ix, rows_idx, dim, bits, metric, q):
    out = []
    for r in rows_idx:
        raw = ix.read_rows(int(r), 1)
        out.append(orc.all_distances(raw, dim, bits, metric, q)[0])
    return np.array(out)


@pytest.mark.parametrize("name,n,dim,bits,metric,k", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_fullsize_properties(name, n, dim, bits, metric, k):
    seed = 0x53595A4700000100 + len(name)
    Q = synth_vectors(seed + 1, 0, 3, dim)
    with ScanIndex(dim, bits, metric) as ix:
        ix.synth(n, seed)
        assert ix.rows == n
        # device-side synthesis == oracle synthesis on a window in the middle
        assert (ix.read_rows(n // 2, 4) == orc.synth_rows(seed, n // 2, 4, dim, bits)).all()
        r, d, c = ix.search_topk(Q, k)
        r100, d100, c100 = ix.search_topk(Q, max(100, k))
        st = ix.stats()
        for qi in range(Q.shape[0]):
            assert c[qi] == k
            assert (np.diff(d[qi]) >= 0).all()
            assert (r100[qi, :k] == r[qi]).all() and (d100[qi, :k] == d[qi]).all()
            want = oracle_dist_for(ix, r[qi], dim, bits, metric, Q[qi])
            assert (want == d[qi]).all(), (want, d[qi])            # bit-exact float64
            # sample of other rows: none may beat the k-th distance
            rng = np.random.default_rng(qi)
            sample = rng.integers(0, n, 300)
            block = orc.synth_rows(seed, int(sample.min()), 1, dim, bits)  # warm the oracle
            del block
            sd = np.array([orc.all_distances(orc.synth_rows(seed, int(s), 1, dim, bits), dim, bits,
                                             metric, Q[qi])[0] for s in sample[:60]])
            inside = set(int(x) for x in r[qi])
            for s, dist in zip(sample[:60], sd):
                if int(s) not in inside:
                    assert dist >= d[qi, k - 1]
        # radius at the k-th distance returns the same leading rows
        rr, dd = ix.search_radius(Q[0], float(d[0, k - 1]))
        assert len(rr) >= k and (rr[:k] == r[0]).all() and (dd[:k] == d[0]).all()
        # a stored row as the query comes back first (distance 0, or NaN/tiny for cosine)
        target = n - 7
        stored = orc.decode_vector(ix.read_rows(target, 1)[0], dim, bits)
        r1, d1, _ = ix.search_topk(stored, 1)
        o = orc.all_distances(ix.read_rows(target, 1), dim, bits, metric, stored)[0]
        if not np.isnan(o):
            assert int(r1[0, 0]) == target and d1[0, 0] == o
        assert st["escalations"] == 0 or name.startswith("cfg5")


def test_headline_full_oracle_scan_one_query():
    """One full 1M x 768 oracle scan (a few seconds of CPU) against the HIP answer."""
    n, dim, bits, metric, k = 1_000_000, 768, 32, 1, 10
    seed = 0x53595A4700000200
    q = synth_vectors(seed + 1, 0, 1, dim)
    with ScanIndex(dim, bits, metric) as ix:
        ix.synth(n, seed)
        r, d, c = ix.search_topk(q, k)
        rows = ix.read_rows(0, n)
    o_rows, o_dist, searched = orc.search_exact(rows, dim, bits, metric, q[0], k=k)
    assert searched == n
    assert [int(x) for x in r[0]] == [int(x) for x in o_rows]
    assert (d[0] == o_dist).all()
    rel = np.abs(d[0] - o_dist) / o_dist
    assert (rel <= 1e-5).all()   # the contract's tolerance; bit-equality above is stronger


@pytest.mark.parametrize("name,n,dim,bits,metric,k", [c for c in CONFIGS if c[0] in ("cfg2", "cfg3")], ids=["cfg2", "cfg3"])
def test_cfg2_cfg3_full_oracle_scan_one_query(name, n, dim, bits, metric, k):
    """One complete oracle scan of the million rows (1.5 GB / 0.77 GB: seconds of CPU) per configuration against
    the HIP answers for the same query: alone (one sweep per query) and inside a batch (the shared sweep on the
    matrix cores: bfloat16 MFMA for cfg2's float rows, int8 MFMA for cfg3's 8-bit rows)."""
    seed = 0x53595A4700000400 + bits
    Q = synth_vectors(seed + 1, 0, 5, dim)
    with ScanIndex(dim, bits, metric) as ix:
        ix.synth(n, seed)
        ix.set_option("multi_query", 0)
        r1, d1, _ = ix.search_topk(Q[2], k)
        ix.set_option("multi_query", 1)
        rb, db, _ = ix.search_topk(Q, k)
        assert ix.stats()["mq_queries"] == 5
        rows = ix.read_rows(0, n)
    o_rows, o_dist, searched = orc.search_exact(rows, dim, bits, metric, Q[2], k=k)
    assert searched == n
    for r, d in ((r1[0], d1[0]), (rb[2], db[2])):
        assert [int(x) for x in r] == [int(x) for x in o_rows]
        assert (d == o_dist).all()                       # the reference's float64 values bit for bit
        assert (np.abs(d - o_dist) <= 1e-5 * o_dist).all()   # the contract's tolerance


def test_cfg5_full_radius_search():
    """Config #5 as named: 100M x 384 4-bit cosine, radius search (one card holds the
    19.2 GB).  Every hit's distance is the oracle's for that row and <= R; sampled
    non-hits are farther; hits ascend; the hit count is in the calibrated range
    (R chosen for 10^2..10^3 hits)."""
    n, dim, bits, metric = 100_000_000, 384, 4, 1
    seed = 0x53595A4700000300
    R = 0.426
    q = synth_vectors(seed + 1, 0, 2, dim)
    with ScanIndex(dim, bits, metric) as ix:
        ix.synth(n, seed)
        assert (ix.read_rows(n - 3, 3) == orc.synth_rows(seed, n - 3, 3, dim, bits)).all()
        for qi in range(2):
            rows, dist = ix.search_radius(q[qi], R)
            assert 10 <= len(rows) <= 20000, len(rows)
            assert (dist <= R).all()
            want = oracle_dist_for(ix, rows[:50], dim, bits, metric, q[qi])
            assert (want == dist[:50]).all()
            srt = np.sort(dist, kind="stable")
            assert (srt == dist).all() or len(set(dist.tolist())) < len(dist)  # ascending (ties: heap order)
            hits = set(int(x) for x in rows)
            rng = np.random.default_rng(qi)
            for s in rng.integers(0, n, 80):
                dd = orc.all_distances(orc.synth_rows(seed, int(s), 1, dim, bits), dim, bits, metric, q[qi])[0]
                assert (dd <= R) == (int(s) in hits)
            # the k nearest by top-k search are the head of the radius result
            r10, d10, _ = ix.search_topk(q[qi], 10)
            assert (d10[0] <= R).all() and set(int(x) for x in r10[0]) <= hits


# ---- step compaction of selective masks at scale (kernels_scan.hip, general phase) ---------------------------------------
# A wave under a selective mask first compacts the row steps that hold a passing row into its LDS step list, 64 steps
# per loop iteration, and rings over the list once it holds more than 192 entries (or the steps are used up); what is
# left goes into further rounds.  Small corpora give a wave a handful of steps: one iteration, one round.  Here a cell
# with ONE row per wave step (L = 64) gets so many rows that every wave has more than 256 steps.

COMPACT_STEPS = 300   # row steps per wave: > 64 (a second loop iteration), > 256 (steps are left for a second round)


def _compaction_cell():
    """64-bit rows, one row per wave step: the lattice's L = 64, P = 1 cell (the fewest elements per row for the oracle)."""
    c = next(c for c in lat.cells(64) if c.L == 64 and c.P == 1)
    p = scan_plan(c.dim, 64, 1 << 40, lat.kp_of(10), masked=True)
    assert p["gpw"] == 1 and p["rows_per_block"] == p["block"] // 64
    stride = p["grid"] * p["rows_per_block"]          # rows between two steps of a wave
    return c, stride, COMPACT_STEPS * stride + 1      # (+1: a partial mask word, and one wave with a step more)


_compaction_kept = {}


def _compaction_corpus():
    if not _compaction_kept:
        c, stride, n = _compaction_cell()
        seed = 0x53595A4700000500
        ix = ScanIndex(c.dim, 64, 1)
        ix.synth(n, seed)
        ix.set_option("multi_query", 0)
        ix.set_option("sketch", 0)
        _compaction_kept.update(ix=ix, rows=ix.read_rows(0, n), q=synth_vectors(seed + 1, 0, 1, c.dim)[0], seed=seed)
        assert (_compaction_kept["rows"][n - 3:] == orc.synth_rows(seed, n - 3, 3, c.dim, 64)).all()
    return _compaction_kept


@pytest.mark.parametrize("form", ["second-iteration", "second-round"])
def test_step_compaction_at_scale(form):
    """second-iteration: a 2 % filter over 300 steps per wave -- the compaction loop runs five iterations and lists
    about six steps.  second-round: a 90 % filter with the dense masked form switched off -- the first 256 steps of a
    wave list more than 192 passing ones, the ring runs, and the rest is compacted in a second round.  One query each,
    against a complete oracle scan."""
    c, stride, n = _compaction_cell()
    kept = _compaction_corpus()
    ix, rows, q = kept["ix"], kept["rows"], kept["q"]
    rng = np.random.default_rng(5)
    allow = rng.random(n) < (0.02 if form == "second-iteration" else 0.9)
    per_wave = allow[: COMPACT_STEPS * stride].reshape(COMPACT_STEPS, stride)   # [step, wave]: gpw == 1
    p = scan_plan(c.dim, 64, n, lat.kp_of(10), masked=True)
    assert p["grid"] * p["rows_per_block"] == stride   # the grid is at its cap
    if form == "second-iteration":
        assert COMPACT_STEPS > 64 and per_wave.sum(axis=0).max() <= 192     # several iterations, one round
        ix.set_option("mask_dense", 1)                                     # (selective by its pass rate)
    else:
        first = per_wave[:256].sum(axis=0)
        assert COMPACT_STEPS > 256 and (first > 192).mean() > 0.99, first.min()   # a second round in nearly every wave
        ix.set_option("mask_dense", 0)
    ix.reset_stats()
    r, d, cnt = ix.search_topk(q, 10, allow=allow)
    with ix.mask(allow) as m:
        rm, dm, cm = ix.search_topk(q, 10, masks=m)
        hits = ix.search_radius(q, float(d[0, 9]), masks=m)
    st = ix.stats()
    assert st["mq_queries"] == 0 and st["sketch_queries"] == 0 and st["scan_launches"] > 0, st
    o_rows, o_dist, _ = orc.search_exact(rows, c.dim, 64, 1, q, k=10, allow=allow.astype(np.uint8))
    for got_r, got_d in ((r[0, : cnt[0]], d[0, : cnt[0]]), (rm[0, : cm[0]], dm[0, : cm[0]]), (hits[0][:10], hits[1][:10])):
        assert [int(x) for x in got_r] == [int(x) for x in o_rows]
        assert (np.asarray(got_d) == o_dist).all()
    assert len(hits[0]) == 10 or hits[1][10] == hits[1][9]
    if form == "second-round":   # the last form: the shared handle goes
        ix.close()
        _compaction_kept.clear()
