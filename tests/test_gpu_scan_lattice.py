"""The one-sweep scan kernel (kernels_scan.hip) over its whole shape lattice, against the CPU oracle.

tests/scan_lattice.py derives one cell per lane-map class and per row-shape-specialised kernel from the library's own
launch rules; here every cell is searched at a small row count under every launch variant (top-k with register and
LDS lists, collect, dense and selective masks, tombstones, filters from the host and resident on the card) and at a
deep row count where every wave walks several rows in the predicate-free dense phase.  Row-count edges and the largest
dimension of each width follow.

Every test forces the kernel under test (multi_query = 0, sketch = 0) and checks from the statistics that it served.
Rows and order must be the oracle's, float64 distances bit-equal (NaN == NaN): no tolerance.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as orc
import scan_lattice as lat
from syzgydb_amd import ScanIndex, SzgError
from syzgydb_amd._lib import SZG_E_UNSUPPORTED

pytestmark = pytest.mark.gpu

SEED = 0x53595A4700001000
METRICS = (0, 1)   # Euclidean, cosine
CELLS = lat.all_cells()
CELL_METRIC = [(c, m) for c in CELLS for m in METRICS]
CELL_METRIC_IDS = ["%s-%s" % (lat.cell_id(c), "cos" if m else "euc") for c, m in CELL_METRIC]
POOL = ThreadPoolExecutor(8)   # the oracle's C calls release the interpreter lock


def assert_same(got_rows, got_dist, want, what):
    want_rows, want_dist = want
    assert [int(x) for x in got_rows] == [int(x) for x in want_rows], ("rows differ", what)
    g, w = np.asarray(got_dist, dtype=np.float64), np.asarray(want_dist, dtype=np.float64)
    assert ((g == w) | (np.isnan(g) & np.isnan(w))).all(), ("distances not bit-equal", what, g, w)


def open_index(dim, bits, metric, n, seed):
    ix = ScanIndex(dim, bits, metric)
    ix.synth(n, seed)
    ix.set_option("multi_query", 0)   # one sweep per query: the kernel under test
    ix.set_option("sketch", 0)
    return ix


def assert_scan_kernel_served(ix):
    st = ix.stats()
    assert st["mq_queries"] == 0 and st["sketch_queries"] == 0 and st["scan_launches"] > 0, st


def cell_seed(c):
    return SEED + c.bits * 100000 + c.r16 * 16


def check_topk(ix, Q, ks, want, what, **filt):
    got = {}
    for k in ks:
        r, d, cnt = ix.search_topk(Q, k, **filt)
        for qi in range(Q.shape[0]):
            assert_same(r[qi, : cnt[qi]], d[qi, : cnt[qi]], want[k][qi], (what, "k", k, "query", qi))
        got[k] = (r, d, cnt)
    return got


def check_radius(ix, Q, radii, want, what, **filt):
    hits = ix.search_radius_batch(Q, radii, **filt)
    for qi in range(Q.shape[0]):
        assert_same(hits[qi][0], hits[qi][1], want[qi], (what, "radius", radii[qi], "query", qi))
    return hits


class Reference:
    """The oracle's answers for one corpus and its queries, computed once per effective mask and kept."""

    def __init__(self, rows, dim, bits, metric, Q, ks, radii):
        self.rows, self.dim, self.bits, self.metric, self.Q, self.ks, self.radii = rows, dim, bits, metric, Q, ks, radii
        self._kept = {}

    def answers(self, name, masks):
        """masks: one bool[n] (or None) per query.  -> ({k: [(rows, dist) per query]}, [(rows, dist) per query])"""
        if name not in self._kept:
            topk = {k: [] for k in self.ks}
            rad = []
            for qi, m in enumerate(masks):
                a = None if m is None else m.astype(np.uint8)
                for k in self.ks:
                    topk[k].append(orc.search_exact(self.rows, self.dim, self.bits, self.metric, self.Q[qi], k=k, allow=a)[:2])
                rad.append(orc.search_exact(self.rows, self.dim, self.bits, self.metric, self.Q[qi], radius=self.radii[qi],
                                            allow=a)[:2])
            self._kept[name] = (topk, rad)
        return self._kept[name]


def sub(want, idx):
    topk, rad = want
    return {k: [v[i] for i in idx] for k, v in topk.items()}, [rad[i] for i in idx]


# ---- small n: every launch variant ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell,metric", CELL_METRIC, ids=CELL_METRIC_IDS)
def test_small_rows_every_variant(cell, metric):
    """Three queries per call (the query-major loop moves on to a second and third query), k = 1, 10 and 80 (80: lists
    in LDS, the deep ring) and one radius batch (collect), each unfiltered, under a mild and a selective filter, with
    tombstones, and with both -- the masked ones also with the dense masked form switched off, and every filter both as
    host words (allow=) and as resident masks (masks=: differing handles are gathered into slots, one shared handle is
    read in place with stride 0)."""
    bits, dim, n = cell.bits, cell.dim, cell.small_n
    seed = cell_seed(cell)
    rows = orc.synth_rows(seed, 0, n, dim, bits)
    Q = orc.synth_vectors(seed + 1, 0, 3, dim)
    radii = []
    for q in Q:
        alld = orc.all_distances(rows, dim, bits, metric, q)
        radii.append(float(np.quantile(alld[np.isfinite(alld)], 0.05)))
    assert all(r > 0 for r in radii), radii
    ref = Reference(rows, dim, bits, metric, Q, lat.KS, radii)
    rng = np.random.default_rng(seed & 0xFFFFFFFF)
    filters = {}
    for name, rate in (("allow 0.9", 0.9), ("allow 0.02", 0.02)):
        a = rng.random(n) < rate
        a[int(rng.integers(0, n))] = True            # never empty
        filters[name] = [a, np.roll(a, 1), a]        # queries 0 and 2 share a mask, query 1 has its own
    live = np.ones(n, dtype=bool)
    dead = np.arange(n) % 7 == 3                     # 1/7 of the rows
    with open_index(dim, bits, metric, n, seed) as ix:
        assert (ix.read_rows(n - 1, 1) == rows[n - 1:]).all()   # device synthesis == the oracle's

        def filtered(name, tag):
            per_query = filters[name]
            want = ref.answers(name + tag, [m & live for m in per_query])
            A, B = ix.mask(per_query[0]), ix.mask(per_query[1])
            for md in (1, 0):
                ix.set_option("mask_dense", md)
                what = (lat.cell_id(cell), name + tag, "mask_dense", md)
                host = check_topk(ix, Q, lat.KS, want[0], what + ("allow=",), allow=np.stack(per_query))
                check_radius(ix, Q, radii, want[1], what + ("allow=",), allow=np.stack(per_query))
                res = check_topk(ix, Q, lat.KS, want[0], what + ("masks=[A, B, A]",), masks=[A, B, A])
                check_radius(ix, Q, radii, want[1], what + ("masks=[A, B, A]",), masks=[A, B, A])
                for k in lat.KS:   # the same filter from the host and from the card: the same answer
                    (hr, hd, hc), (mr, md_, mc) = host[k], res[k]
                    assert (hr == mr).all() and (hc == mc).all() and ((hd == md_) | (np.isnan(hd) & np.isnan(md_))).all()
                w02 = sub(want, [0, 2])
                check_topk(ix, Q[[0, 2]], lat.KS, w02[0], what + ("masks=A",), masks=A)
                check_radius(ix, Q[[0, 2]], [radii[0], radii[2]], w02[1], what + ("masks=A",), masks=A)
            ix.set_option("mask_dense", 1)
            A.close()
            B.close()

        want = ref.answers("none", [None] * 3)
        check_topk(ix, Q, lat.KS, want[0], (lat.cell_id(cell), "unfiltered"))
        check_radius(ix, Q, radii, want[1], (lat.cell_id(cell), "unfiltered"))
        filtered("allow 0.9", "")
        filtered("allow 0.02", "")
        for r in np.flatnonzero(dead):
            ix.tombstone(int(r))
        live = ~dead
        assert ix.live_rows == int(live.sum())
        want = ref.answers("tombstones", [live] * 3)
        for md in (1, 0):
            ix.set_option("mask_dense", md)
            check_topk(ix, Q, lat.KS, want[0], (lat.cell_id(cell), "tombstones", "mask_dense", md))
            check_radius(ix, Q, radii, want[1], (lat.cell_id(cell), "tombstones", "mask_dense", md))
        filtered("allow 0.9", " + tombstones")
        assert_scan_kernel_served(ix)


# ---- deep n: the dense phase over several rows per wave ------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def deep_corpus(bits, r16, dim, n, seed):
    """The oracle's copy of a deep cell's rows, synthesised in slices side by side; shared by the cell's two metrics."""
    cuts = np.linspace(0, n, 9).astype(np.int64)
    parts = POOL.map(lambda i: orc.synth_rows(seed, int(cuts[i]), int(cuts[i + 1] - cuts[i]), dim, bits), range(8))
    return np.concatenate(list(parts))


@pytest.mark.parametrize("cell,metric", CELL_METRIC, ids=CELL_METRIC_IDS)
def test_deep_rows_dense_phase(cell, metric):
    """Every wave walks ceil(2 * D / P) + 2 row steps (tests/test_scan_plan_cpu.py checks that from the plan): the
    predicate-free dense phase with its pointer-increment addressing runs over several rows per wave, then hands the
    last step to the general phase.  Unfiltered (row ids after the row jump), a 0.9 filter as a resident mask
    (the dense phase's mask words), a 0.02 filter (step compaction) and one radius search (the collect variant)."""
    bits, dim, n, k = cell.bits, cell.dim, cell.deep_n, lat.DEEP_K
    seed = cell_seed(cell) + 7
    rows = deep_corpus(bits, cell.r16, dim, n, seed)
    q = orc.synth_vectors(seed + 1, 0, 1, dim)[0]
    rng = np.random.default_rng(seed & 0xFFFFFFFF)
    a9, a02 = rng.random(n) < 0.9, rng.random(n) < 0.02
    # a radius with a few hundred to a few thousand hits: the k-th distance within the first 4096 rows
    head = orc.search_exact(rows[:4096], dim, bits, metric, q, k=k)[1]
    radius = float(head[np.isfinite(head)][-1])
    assert radius > 0
    jobs = [POOL.submit(orc.search_exact, rows, dim, bits, metric, q, k=k),
            POOL.submit(orc.search_exact, rows, dim, bits, metric, q, k=k, allow=a9.astype(np.uint8)),
            POOL.submit(orc.search_exact, rows, dim, bits, metric, q, k=k, allow=a02.astype(np.uint8)),
            POOL.submit(orc.search_exact, rows, dim, bits, metric, q, radius=radius)]
    with open_index(dim, bits, metric, n, seed) as ix:
        for at in (0, n // 2, n - 2):
            assert (ix.read_rows(at, 2) == rows[at:at + 2]).all()
        r0, d0, c0 = ix.search_topk(q, k)
        with ix.mask(a9) as m9:
            r9, d9, c9 = ix.search_topk(q, k, masks=m9)
        r2, d2, c2 = ix.search_topk(q, k, allow=a02)
        rr, dd = ix.search_radius(q, radius)
        assert_scan_kernel_served(ix)
    what = lat.cell_id(cell)
    assert_same(r0[0, : c0[0]], d0[0, : c0[0]], jobs[0].result()[:2], (what, "unfiltered"))
    assert_same(r9[0, : c9[0]], d9[0, : c9[0]], jobs[1].result()[:2], (what, "resident mask 0.9"))
    assert_same(r2[0, : c2[0]], d2[0, : c2[0]], jobs[2].result()[:2], (what, "allow 0.02"))
    assert_same(rr, dd, jobs[3].result()[:2], (what, "radius", radius))


# ---- row-count edges ------------------------------------------------------------------------------------------------------

EDGE = [(c, m) for bits in lat.WIDTHS for c in lat.edge_cells(bits) for m in METRICS]


@pytest.mark.parametrize("cell,metric", EDGE, ids=["%s-%s" % (lat.cell_id(c), "cos" if m else "euc") for c, m in EDGE])
def test_row_count_edges(cell, metric):
    """n = 1, one row short of / exactly / one row past a wave step, and one row either side of a block's rows; a
    filter that allows only the LAST row, a tombstone on row 0 only, and both."""
    bits, dim = cell.bits, cell.dim
    seed = cell_seed(cell) + 3
    Q = orc.synth_vectors(seed + 1, 0, 3, dim)
    for n in lat.edge_rows(cell):
        rows = orc.synth_rows(seed, 0, n, dim, bits)
        ref = Reference(rows, dim, bits, metric, Q, (1, 10), [1000.0] * 3)   # (a radius that takes every row)
        last = np.zeros(n, dtype=bool)
        last[n - 1] = True
        live = np.ones(n, dtype=bool)
        with open_index(dim, bits, metric, n, seed) as ix:
            what = (lat.cell_id(cell), "n", n)
            want = ref.answers("none", [None] * 3)
            check_topk(ix, Q, (1, 10), want[0], what)
            check_radius(ix, Q, [1000.0] * 3, want[1], what)
            for stage in ("", " + tombstone on row 0"):
                if stage:
                    ix.tombstone(0)
                    live[0] = False
                    want = ref.answers("dead0", [live] * 3)
                    check_topk(ix, Q, (1, 10), want[0], what + (stage,))
                want = ref.answers("last" + stage, [last & live] * 3)
                with ix.mask(last) as m:
                    for md in (1, 0):
                        ix.set_option("mask_dense", md)
                        check_topk(ix, Q, (1, 10), want[0], what + ("only the last row" + stage, md), allow=np.stack([last] * 3))
                        check_topk(ix, Q, (1, 10), want[0], what + ("only the last row, resident" + stage, md), masks=m)
                        check_radius(ix, Q, [1000.0] * 3, want[1], what + ("only the last row, resident" + stage, md), masks=m)
                for qi in range(3):
                    assert len(want[0][10][qi][0]) == (0 if (n == 1 and stage) else 1)
            assert_scan_kernel_served(ix)


# ---- the largest dimension ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS, ids=["euc", "cos"])
@pytest.mark.parametrize("bits", lat.WIDTHS)
def test_largest_dimension(bits, metric):
    """The largest dimension szg_index_create accepts (48 KiB of prepared query in LDS) answers correctly with lists in
    registers (k = 10) and in LDS beside that query (k = 80); one 16-byte piece more is refused."""
    dim = lat.max_dim(bits)
    p = lat.scan_plan(dim, bits, 1 << 22, lat.kp_of(10))
    n = lat.small_rows(p)
    seed = SEED + 900 + bits
    rows = orc.synth_rows(seed, 0, n, dim, bits)
    Q = orc.synth_vectors(seed + 1, 0, 2, dim)
    ref = Reference(rows, dim, bits, metric, Q, (10, 80), [1000.0] * 2)
    with open_index(dim, bits, metric, n, seed) as ix:
        check_topk(ix, Q, (10, 80), ref.answers("none", [None] * 2)[0], ("largest dim", bits, dim))
        assert_scan_kernel_served(ix)
    with pytest.raises(SzgError) as e:
        ScanIndex(dim + lat.elements_per_piece(bits), bits, metric)
    assert e.value.code == SZG_E_UNSUPPORTED
