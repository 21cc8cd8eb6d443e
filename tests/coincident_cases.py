"""Corpora with queries at and near stored rows: what tests/test_gpu_coincident.py searches and tests/test_coincident_cpu.py
checks with the oracle alone.  Test support, like scan_lattice.py.

A case starts from orc.synth_rows, 16 m + 5 rows with m the largest that keeps nq * n * dim within cert_check.WIDE_LIMIT
(2 005 rows at the most): cert_check.Corpus.keys then computes every real-number key in the element-by-element difference
form, whose error is relative to the key -- the expanded form's absolute error would be larger than a key at zero.  Rows
are planted by overwriting packed rows; the queries that go with them take the first positions of the batch, the rest
is orc.synth_vectors:

    Q[0]  P0   decode(r0): the real-number key is exactly 0.  Three byte-identical copies of r0 sit in the first tile,
               mid-corpus and in the partial last tile: four rows at distance 0
    Q[1]  P1   decode(r1) + d, |d_i| <= 1/4 of the spacing at the prepared element: the prepared query rounds to the row
    Q[2]  P2   decode(r2a) moved by 1 spacing in 1 coordinate
    Q[3]  P2   decode(r2b) moved by 3 spacings in 7 coordinates
    Q[4]  P2   decode(r2c) moved by 17 spacings in every coordinate (r2c lies in the partial last tile)

The spacing: float32's at x_i for 32- and 64-bit rows (the shared sweeps narrow 64-bit rows to float32), float32's at
65535 x_i for 16-bit rows, the query's quantization step max|x| / Qmax of the path under test for 8- and 4-bit rows.
far: the corpus and the queries shifted by +1 000 in every coordinate (32- and 64-bit rows).
"""

import numpy as np

import oracle as orc
from syzgydb_amd import cert_check as cc

SEED = 0x53595A4700012000
MAX_ROWS = 2005
TINY = 5e-324   # the smallest positive radius: "radius 0" (a radius of 0 itself means "no radius" and is refused)
RADIUS_KINDS = ("smallest positive", "the near row's distance", "just under the near row's distance", "1e-12", "some tens of rows")
# largest |Q| of the integer queries: one-sweep 8-bit (three planes), one-sweep 4-bit (kQmax4), the int8 shared sweep
QMAX_ONE_SWEEP = {8: 1000000.0, 4: 30000.0}
QMAX_SHARED = 16000.0


def n_rows(nq, dim):
    m = min((MAX_ROWS - 5) // 16, (cc.WIDE_LIMIT // (nq * dim) - 5) // 16)
    n = 16 * m + 5
    assert n >= 1500 and nq * n * dim <= cc.WIDE_LIMIT, (nq, n, dim)
    return n


def f32_spacing(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def spacing(x, bits, qmax):
    """Per element of a query at the decoded row x, in the query's units."""
    if bits >= 32:
        return f32_spacing(x)
    if bits == 16:
        return f32_spacing(65535.0 * x) / 65535.0
    return np.full(x.shape, np.abs(x).max() / qmax)


class Case:
    def __init__(self, corpus, Q, planted, copies, r0):
        self.corpus, self.Q, self.planted, self.copies, self.r0 = corpus, Q, planted, copies, r0
        self.lone = cc.Corpus(corpus.packed, corpus.dim, corpus.bits, corpus.metric)   # (keys of one query at a time)
        self._dists = None

    @property
    def pairs(self):
        """Every (query, row) pair the case exists for: the planted ones and (0, copy) for each copy of r0."""
        return [(qi, row) for qi, row, _ in self.planted] + [(0, c) for c in self.copies]

    @property
    def planted_rows(self):
        return sorted({row for _, row in self.pairs})

    def with_metric(self, metric):
        return Case(self.corpus.with_metric(metric), self.Q, self.planted, self.copies, self.r0)

    def dists(self):
        """The oracle's float64 distance of every (query, row)."""
        if self._dists is None:
            c = self.corpus
            self._dists = np.stack([orc.all_distances(c.packed, c.dim, c.bits, c.metric, q) for q in self.Q])
        return self._dists

    def keep_mask(self):
        """A mask that keeps 60 % of the rows and every planted one."""
        allow = np.random.default_rng(self.corpus.n + self.corpus.dim).random(self.corpus.n) < 0.6
        allow[self.planted_rows] = True
        return allow

    def radii(self, kind, eligible=None):
        """One radius per query of RADIUS_KINDS[kind]; the near row is the nearest eligible row of the oracle."""
        out = np.empty(self.Q.shape[0])
        for qi, d in enumerate(self.dists()):
            s = np.sort(d[np.isfinite(d) & (True if eligible is None else np.broadcast_to(eligible, (self.Q.shape[0], d.size))[qi])])
            near = float(s[0])
            if kind == 0:
                out[qi] = TINY
            elif kind == 1:
                out[qi] = near if near > 0 else TINY
            elif kind == 2:
                under = float(np.nextafter(near, 0.0))
                out[qi] = under if under > 0 else 1e-300
            elif kind == 3:
                out[qi] = 1e-12
            else:
                out[qi] = (s[30] + s[31]) / 2
        return out


def build(bits, dim, nq, metric, qmax=None, far=False):
    assert nq >= 5 and (not far or bits >= 32)
    n = n_rows(nq, dim)
    seed = SEED + bits * 100000 + dim * 16 + (7 if far else 0)
    rows = orc.synth_rows(seed, 0, n, dim, bits).copy()
    Q = orc.synth_vectors(seed + 1, 0, nq, dim)
    if far:
        rows = orc.encode_rows(cc.decode_rows(rows, dim, bits) + 1000.0, bits)
        Q += 1000.0
    r0, copies = 211, (5, (n // 2) | 1, n - 2)
    r1, r2a, r2b, r2c = 402, 1107, 1203, n - 4   # (the mid-corpus copy lies in 751 .. 1003)
    for c in copies:
        rows[c] = rows[r0]
    corpus = cc.Corpus(rows, dim, bits, metric)
    corpus.check_decode(orc, at=[r0, r1, n - 1])
    rng = np.random.default_rng(seed & 0xFFFFFFFF)

    def decoded(r):
        x = orc.decode_vector(rows[r], dim, bits)
        return x, spacing(x, bits, qmax)

    Q[0] = decoded(r0)[0]
    x, sp = decoded(r1)
    Q[1] = x + rng.uniform(-0.25, 0.25, dim) * sp
    for qi, r, move, coords in ((2, r2a, 1, 1), (3, r2b, 3, 7), (4, r2c, 17, dim)):
        x, sp = decoded(r)
        at = rng.choice(dim, min(coords, dim), replace=False)
        x[at] += rng.choice((-1.0, 1.0), at.size) * move * sp[at]
        Q[qi] = x
    planted = [(0, r0, "P0"), (1, r1, "P1"), (2, r2a, "P2"), (3, r2b, "P2"), (4, r2c, "P2")]
    assert corpus.finite.all() and (cc.decode_rows(rows, dim, bits) != 0).any(axis=1).all()   # no non-finite element, no zero row
    return Case(corpus, Q, planted, copies, r0)


def float32_key(case, qi, row):
    """The one-sweep kernel's Euclidean key of (query, row) on 32- and 16-bit rows if its float32 sum were exact: the
    prepared query narrowed to float32, less the row's elements (exact in float32), squared and summed in float64.  It is
    0 exactly when every float32 difference is, whatever the order of the sum."""
    c = case.corpus
    assert c.bits in (16, 32)
    x = c.rows(row, row + 1)[0]
    if c.bits == 16:
        x = np.rint((x + 1) / 2 * 65535.0) * 2 - 65535.0   # n = 2 v - 65535
    g = (case.Q[qi] * c.scale).astype(np.float32)
    d = g - x.astype(np.float32)
    return float((d.astype(np.float64) ** 2).sum())


# ---- the cosine leg: queries parallel to a stored row -----------------------------------------------------------------

def build_parallel(bits, dim, nq, k_split=10):
    """Q = c decode(r) for c in (1, 0.5, 3) and one query a few spacings off parallel, for r planted once below row
    k_split and once above it: the reference's unclamped acos gives 0 or NaN at such a pair.  -> Case (cosine)"""
    assert nq >= 8
    n = n_rows(nq, dim)
    seed = SEED + 900000 + bits * 1000 + dim
    rows = orc.synth_rows(seed, 0, n, dim, bits).copy()
    Q = orc.synth_vectors(seed + 1, 0, nq, dim)
    lo, hi = 3, n - 3
    assert lo < k_split < hi
    planted = []
    for base, r in ((0, lo), (4, hi)):
        x = orc.decode_vector(rows[r], dim, bits)
        for j, c in enumerate((1.0, 0.5, 3.0)):
            Q[base + j] = c * x
            planted.append((base + j, r, "parallel"))
        off = x.copy()
        off[: min(3, dim)] += 5 * spacing(x, bits, QMAX_SHARED)[: min(3, dim)]
        Q[base + 3] = off
        planted.append((base + 3, r, "near parallel"))
    return Case(cc.Corpus(rows, dim, bits, 1), Q, planted, (), lo)
