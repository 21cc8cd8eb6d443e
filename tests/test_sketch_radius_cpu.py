"""Radius searches through the 8-bit sketch (option sketch_radius), host only: the option's range, the plan hook of the
matrix sweep's collect form (szg_debug_scan_collect: scan_variant's answer for collect launches of the sketch) and the
rules cert_check applies to the new certificate pass -- K_s, C_s, T, S_r -- each against a hand-built record that breaks
it, so that every rule is seen to fail.

Documented LDS of the collect form (include/syzgy_scan.h): with b column blocks 16 b (2 dim64 + 16) bytes -- the images
and four words per query (qscale, qconst, qnorm2, threshold), no lists."""
import numpy as np
import pytest

from syzgydb_amd import SzgError, _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import option_check, scan_collect_plan, scan_matrix_plan

DIMS = (64, 192, 384, 768)
STEPS = {64: 0, 192: 0, 384: 6, 768: 12}
NOT_SERVED = (("masked", dict(masked=True)), ("three planes", dict(planes=3)), ("untiled", dict(tiled=False)),
              ("no norms", dict(norms=False)), ("scan_group = 4", dict(scan_group=4)), ("scan_group = 1", dict(scan_group=1)),
              ("sketch_matrix = 1", dict(sketch_matrix=1)))


def lds_bytes(dim, blocks):
    return 16 * blocks * (2 * ((dim + 63) // 64 * 64) + 16)


def test_option_range():
    for v in (0, 1):
        option_check("sketch_radius", v)
    for v in (-1, 2, 3):
        with pytest.raises(SzgError, match="sketch_radius is 0 or 1"):
            option_check("sketch_radius", v)


@pytest.mark.parametrize("dim", DIMS)
def test_serves_collect_launches_of_three_queries_or_more(dim):
    for nq in (3, 4, 15, 16, 17, 33, 40):
        p = scan_collect_plan(dim, 8, nq)
        assert p["serves"] and not p["wide"], (dim, nq, p)
        assert p["steps"] == STEPS[dim] and p["lds_bytes"] == lds_bytes(dim, 1), (dim, nq, p)
    for nq in (1, 2):
        assert scan_collect_plan(dim, 8, nq, sketch_matrix=2)["serves"], (dim, nq)   # whatever the count


@pytest.mark.parametrize("dim", DIMS)
def test_does_not_serve(dim):
    for nq in (1, 2):   # automatic: a lone query (and a pair) keeps the one-query collect kernel, one pass each
        p = scan_collect_plan(dim, 8, nq)
        assert not p["serves"] and p["passes"] == nq, (dim, nq, p)
    for nq in (3, 16, 40):
        for why, kw in NOT_SERVED:
            for wide in (0, 2):
                p = scan_collect_plan(dim, 8, nq, sketch_wide=wide, **kw)
                assert not p["serves"] and not p["wide"] and p["passes"] == nq, (dim, nq, why, p)
    for bits in (4, 16, 32):
        assert not scan_collect_plan(dim, bits, 16, sketch_matrix=2)["serves"], (dim, bits)
    assert not scan_collect_plan(48, 8, 16, sketch_matrix=2)["serves"]   # rows that are no whole 64-byte steps


def test_pass_counts_and_lds():
    for dim in DIMS:
        # launches of up to 16: one pass each; the last launch of 17 and of 33 holds ONE query, which under automatic
        # keeps the one-query kernel -- one pass as well
        assert [scan_collect_plan(dim, 8, nq)["passes"] for nq in (3, 16, 17, 33)] == [1, 1, 2, 3], dim
        # sketch_wide = 2: launches of up to 32
        w = [scan_collect_plan(dim, 8, nq, sketch_wide=2) for nq in (3, 16, 17, 33)]
        assert [p["passes"] for p in w] == [1, 1, 1, 2], dim
        assert [p["wide"] for p in w] == [False, False, True, True], dim
        assert w[2]["lds_bytes"] == lds_bytes(dim, 2) <= 64 * 1024, (dim, w[2])
        assert not scan_collect_plan(dim, 8, 33, sketch_wide=1)["wide"]
    # the two-block form at 768 dimensions: 48 KiB of images and 512 bytes of constants
    assert lds_bytes(768, 2) == 49664
    assert scan_collect_plan(768, 8, 32, sketch_wide=2)["lds_bytes"] == 49664


def test_the_topk_hook_answers_as_before():
    for dim in DIMS:
        m = scan_matrix_plan(dim, 8, 16, kp=8)
        assert m["serves"] and m["passes"] == 1 and m["steps"] == STEPS[dim], (dim, m)
        assert m["lds_bytes"] == 16 * (2 * ((dim + 63) // 64 * 64) + 12 + 8 * 4 * 8), (dim, m)


# ---- cert_check: the sketch-radius pass against hand-built records ------------------------------------------------------

DIM, N, COS = 16, 96, _lib.SZG_COSINE
REC = np.dtype(_lib.SzgCertRecord)
ENT = np.dtype(_lib.SzgCertEntry)
EPS = 1e-4


class World:
    """96 float32 rows (row 5 is all zero: no usable sketch), their 8-bit sketches by cert_check.sketch_reference, one
    query, and a record of pass SZG_CERT_SKETCH_RADIUS that is right in every respect."""

    def __init__(self):
        rng = np.random.default_rng(77)
        V = rng.standard_normal((N, DIM)).astype(np.float32).astype(np.float64)
        V[5] = 0.0
        self.q = rng.standard_normal((1, DIM))
        t, must = cc.sketch_reference(V, COS, 0.0)
        assert list(np.flatnonzero(must)) == [5]
        sk = np.clip(np.rint(t.astype(np.float64)), 0, 255).astype(np.uint8)
        sk[5] = 128
        self.exc = np.array([5], dtype=np.uint64)
        self.corpus = cc.Corpus(V.astype(">f4").view(np.uint8).reshape(N, -1), DIM, 32, COS)
        self.sk_corpus = cc.Corpus(sk, DIM, 8, COS)
        with np.errstate(all="ignore"):
            c = (V @ self.q[0]) / (np.linalg.norm(V, axis=1) * np.linalg.norm(self.q[0]))
            self.dists = (np.arccos(np.clip(c, -1, 1)) / np.pi)[None, :]
            S = 2.0 * sk.astype(np.float64) - 255.0
            cs = (V * S).sum(axis=1) / (np.linalg.norm(V, axis=1) * np.linalg.norm(S, axis=1))
        ang = np.arccos(np.clip(np.delete(cs, 5), -1, 1)) / np.pi
        self.slack = cc.sketch_slack(float(ang.max()), 0.0, DIM)
        d = np.sort(np.delete(self.dists[0], 5))
        self.radius = float((d[9] + d[10]) / 2)   # ten hits
        self.D = self.radius * (1.0 + 1e-9) + self.slack
        self.thr = float(np.float32(-np.cos(np.pi * self.D) + 3 * EPS))
        self.real_s = self.sk_corpus.keys(self.q)[0][0]
        self.rows = [int(r) for r in np.flatnonzero(self.real_s <= self.thr) if r != 5]
        assert len(self.rows) >= 10 and len(self.rows) < N - 8

    def entries(self, rows=None):
        rows = self.rows if rows is None else rows
        e = np.zeros(len(rows) + 1, dtype=ENT)
        for i, r in enumerate(rows):
            key = np.float32(self.real_s[r])
            e[i] = (r, self.dists[0, r], float(key) + EPS, key, 0)
        e[-1] = (5, self.dists[0, 5], 0.0, 0.0, _lib.SZG_CERT_ENTRY_NO_KEY)
        return e

    def record(self, n_entries, **over):
        r = np.zeros(1, dtype=REC)
        r["query"], r["pass_"], r["keys"], r["sweep"], r["certified"], r["k"] = 0, _lib.SZG_CERT_SKETCH_RADIUS, 0, 0, -1, -1
        r["row_lo"], r["row_hi"] = 0, N
        r["thr_min"] = r["kmax"] = np.nan
        r["thr"], r["eps"], r["D"], r["slack"] = self.thr, EPS, self.D, self.slack
        r["first_entry"], r["n_entries"] = 0, n_entries
        for k, v in over.items():
            r[k] = v
        return r

    def check(self, ents=None, eligible=None, dists=None, radii=None, exc=None, **over):
        ents = self.entries() if ents is None else ents
        return cc.check(self.corpus, self.q, self.record(len(ents), **over), ents, 0, eligible=eligible,
                        dists=self.dists if dists is None else dists,
                        sketch=(self.sk_corpus, 0.0, self.exc if exc is None else exc),
                        radii=self.radius if radii is None else radii)


@pytest.fixture(scope="module")
def world():
    return World()


def test_a_right_record_passes(world):
    s = world.check()
    assert s.records == 1 and s.checked == len(world.rows) and s.skipped == 0
    assert s.kinds == {("sketch-radius", "Single", "one-sweep"): 1}


def test_the_pass_needs_its_inputs(world):
    ents = world.entries()
    with pytest.raises(AssertionError, match="need the sketch state"):
        cc.check(world.corpus, world.q, world.record(len(ents)), ents, 0, dists=world.dists, radii=world.radius)
    with pytest.raises(AssertionError, match="need the sketch state"):
        cc.check(world.corpus, world.q, world.record(len(ents)), ents, 0, dists=world.dists,
                 sketch=(world.sk_corpus, 0.0, world.exc))


def test_K_s_can_fail(world):
    ents = world.entries()
    ents["key"][0] -= np.float32(50 * EPS)   # (still under the threshold: only K_s can object)
    ents["ub"][0] = float(ents["key"][0]) + EPS
    with pytest.raises(AssertionError, match="K_s: sketch key outside its bound"):
        world.check(ents)


def test_C_s_can_fail(world):
    deep = min(world.rows, key=lambda r: world.real_s[r])   # far under thr - eps
    with pytest.raises(AssertionError, match="C_s: an eligible sketched row under the threshold was not collected"):
        world.check(world.entries([r for r in world.rows if r != deep]))
    above = int(np.argmax(world.real_s))   # a row whose (right) key is above the threshold, among the keyed entries
    assert world.real_s[above] > world.thr + 10 * EPS
    with pytest.raises(AssertionError, match="C_s: a collected sketch key above the threshold"):
        world.check(world.entries(world.rows + [above]))
    eligible = np.ones(N, dtype=bool)
    eligible[world.rows[3]] = False
    with pytest.raises(AssertionError, match="C_s: a row that is not eligible was collected"):
        world.check(eligible=eligible)
    # a collected row that the sketch state lists as having no usable sketch: its key means nothing
    with pytest.raises(AssertionError, match="C_s: a row without a usable sketch among the keyed entries"):
        world.check(exc=np.array([5, world.rows[0]], dtype=np.uint64))
    ents = world.entries()
    ents["flags"][0] = _lib.SZG_CERT_ENTRY_NO_KEY   # a sketched row among the entries without a key
    with pytest.raises(AssertionError, match="C_s"):
        world.check(ents)


def test_T_can_fail(world):
    # a record whose sketch-distance radius implies a key above thr - eps: the sweep's threshold would not cover it
    with pytest.raises(AssertionError, match="T: thr - eps below the key"):
        world.check(D=world.D + 0.02)
    with pytest.raises(AssertionError, match="T: a radius that is handed over was recorded"):
        world.check(D=1.0)


def test_S_r_can_fail(world):
    with pytest.raises(AssertionError, match="S_r: the sketch-distance radius does not cover"):
        world.check(radii=world.radius + 1e-6)
    # a row outside the entries that the oracle puts within the radius
    out = next(r for r in range(N) if r not in world.rows and r != 5)
    dists = world.dists.copy()
    dists[0, out] = world.radius / 2
    with pytest.raises(AssertionError, match="S_r: a row within the radius is neither an entry nor an exception"):
        world.check(dists=dists)
    dists = world.dists.copy()   # ... but an exception row within the radius is the re-rank's business
    dists[0, 5] = world.radius / 2
    world.check(world.entries()[:-1], dists=dists)


def test_the_constants_and_the_stats_mirror():
    assert _lib.SZG_CERT_SKETCH_RADIUS == 5
    names = [n for n, _ in _lib.SzgStats._fields_]
    assert names[-2:] == ["sketch_radius_queries", "sketch_radius_fallbacks"]
    assert "szg_debug_scan_collect" in _lib.EXPORTS
