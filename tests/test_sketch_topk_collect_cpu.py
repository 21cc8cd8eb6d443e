"""Top-k searches of large k through the 8-bit sketch (option sketch_topk_collect), host only: the option's range, the
constant and the exports, the sample plan hook (szg_debug_sample_plan; csrc/sample_plan.h) -- with the stand-alone program
tests/cpp/test_sample_plan.cpp under the address and undefined-behaviour sanitizers -- and the rules cert_check applies to
the new certificate pass: P, R, S_k and F, each against a hand-built record that breaks only it, so that every rule is
seen to fail, and a right record that passes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from syzgydb_amd import ScanIndex, SzgError, _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import option_check, sample_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_range():
    for v in (0, 1):
        option_check("sketch_topk_collect", v)
    for v in (-1, 2, 3):
        with pytest.raises(SzgError, match="sketch_topk_collect is 0 or 1"):
            option_check("sketch_topk_collect", v)


def test_the_constant_and_the_exports():
    assert _lib.SZG_CERT_SKETCH_TOPK_COLLECT == 6
    assert "szg_index_sketch_topk_stats" in _lib.EXPORTS and "szg_debug_sample_plan" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "szg_index_sketch_topk_stats") and hasattr(L, "szg_debug_sample_plan")
    assert [n for n, _ in _lib.SzgSketchTopkStats._fields_] == ["queries", "fallbacks", "sample_rows", "candidates", "overflows"]
    # szg_stats keeps its layout: the counters live beside it
    assert [n for n, _ in _lib.SzgStats._fields_][-2:] == ["sketch_radius_queries", "sketch_radius_fallbacks"]
    assert cc.PASS_NAMES[6] == "sketch-topk-collect"
    assert hasattr(ScanIndex, "sketch_topk_stats") and ScanIndex.sample_plan(6400, 100)["stride"] == 16


def test_stride_steps_at_exactly_4k_sample_rows():
    # 6400 rows: 400 tiles; every 16th tile is 25 tiles = 400 rows = 4 * 100
    for k, stride, rows in ((100, 16, 400), (101, 8, 800), (200, 8, 800), (201, 4, 1600), (400, 4, 1600), (401, 2, 3200),
                            (800, 2, 3200)):
        p = sample_plan(6400, k, 1, 768)
        assert p["serves"] and p["stride"] == stride and p["sample_rows"] == rows, (k, p)
        cap = 1
        while cap < 8 * k * stride:
            cap *= 2
        assert p["cap"] == cap and p["tiles"] * 16 == p["slots"] and p["key_bytes"] == 4 * p["slots"], (k, p)
    assert not sample_plan(6400, 801, 1, 768)["serves"]


def test_not_served():
    none = dict.fromkeys(("stride", "blocks", "tiles", "sample_rows", "slots", "key_bytes", "cap", "lds_bytes"), 0)
    for why, args in (("below 4 k sample rows", (6400, 801, 1, 768)), ("untiled rows", (20000, 35, 1, 48)),
                      ("three planes", (20000, 35, 1, 64, 8, 3)), ("4-bit rows", (20000, 35, 1, 64, 4)),
                      ("float32 rows", (20000, 35, 1, 64, 32)), ("k beyond the cap", (1 << 20, 2049, 1, 64)),
                      ("an image beyond the LDS", (20000, 35, 1, 2048))):
        p = sample_plan(*args)
        assert not p["serves"] and {k: p[k] for k in none} == none, (why, p)
    assert sample_plan(1 << 20, 2048, 32, 64)["cap"] * 32 == 8 << 20   # the batch limit of every call through the sketch
    assert sample_plan(20000, 35, 1, 1984)["serves"]                   # 31 steps: 62 KiB + 192 bytes of LDS
    with pytest.raises(SzgError):
        sample_plan(20000, 35, 33, 64)


def test_slots_with_a_partial_last_tile():
    p = sample_plan(6399, 99, 1, 64)    # tile 399 holds 15 rows and is not in the sample
    assert (p["tiles"], p["sample_rows"], p["slots"]) == (25, 400, 400), p
    p = sample_plan(6401, 100, 1, 64)   # tile 400 holds one row and is in the sample: 16 slots for it
    assert (p["tiles"], p["sample_rows"], p["slots"]) == (26, 401, 416), p
    p = sample_plan(6401, 100, 17, 64)
    assert p["key_bytes"] == 17 * 416 * 4 and p["blocks"] == 2 and p["lds_bytes"] == 2 * (2048 + 192), p
    assert sample_plan(6401, 100, 16, 768)["lds_bytes"] == 12 * 2048 + 192
    assert sample_plan(6401, 100, 32, 768)["lds_bytes"] == 2 * (12 * 2048 + 192) <= 64 * 1024
    assert sample_plan(6401, 100, 32, 1024)["blocks"] == 1   # two blocks of 16 steps would pass 64 KiB


def test_standalone_sample_plan_program_is_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_sample_plan.cpp"
    exe = str(tmp_path / "test_sample_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_sample_plan.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "sample plan ok" in done.stdout


# ---- cert_check: the sketch-topk-collect pass against hand-built records ----------------------------------------------------

DIM, N, K, COS = 16, 96, 10, _lib.SZG_COSINE
REC = np.dtype(_lib.SzgCertRecord)
ENT = np.dtype(_lib.SzgCertEntry)
EPS = 1e-4


class World:
    """96 float32 rows (row 50 is all zero: no usable sketch), their 8-bit sketches by cert_check.sketch_reference, one
    query, and a record of pass SZG_CERT_SKETCH_TOPK_COLLECT that is right in every respect: kmax is the 12th smallest
    real-number sketch key plus EPS, thr_min the distance it implies plus slack, the sweep's radius D covers it, and the
    entries are every sketched row under the threshold, the exception row and the first K rows."""

    def __init__(self):
        rng = np.random.default_rng(78)
        V = rng.standard_normal((N, DIM)).astype(np.float32).astype(np.float64)
        V[50] = 0.0
        self.q = rng.standard_normal((1, DIM))
        t, must = cc.sketch_reference(V, COS, 0.0)
        assert list(np.flatnonzero(must)) == [50]
        sk = np.clip(np.rint(t.astype(np.float64)), 0, 255).astype(np.uint8)
        sk[50] = 128
        self.exc = np.array([50], dtype=np.uint64)
        self.corpus = cc.Corpus(V.astype(">f4").view(np.uint8).reshape(N, -1), DIM, 32, COS)
        self.sk_corpus = cc.Corpus(sk, DIM, 8, COS)
        with np.errstate(all="ignore"):
            c = (V @ self.q[0]) / (np.linalg.norm(V, axis=1) * np.linalg.norm(self.q[0]))
            self.dists = (np.arccos(np.clip(c, -1, 1)) / np.pi)[None, :]
            S = 2.0 * sk.astype(np.float64) - 255.0
            cs = (V * S).sum(axis=1) / (np.linalg.norm(V, axis=1) * np.linalg.norm(S, axis=1))
        ang = np.arccos(np.clip(np.delete(cs, 50), -1, 1)) / np.pi
        self.slack = cc.sketch_slack(float(ang.max()), 0.0, DIM)
        self.real_s = self.sk_corpus.keys(self.q)[0][0]
        keys = np.sort(np.delete(self.real_s, 50))
        self.kmax = float(keys[11] + EPS)                      # twelve sketched rows at or below it
        self.tau = float(np.arccos(-self.kmax) / np.pi * (1 + 1e-12) + self.slack)
        self.D = self.tau * (1.0 + 1e-9) + self.slack
        self.thr = float(np.float32(-np.cos(np.pi * self.D) + 3 * EPS))
        self.rows = [int(r) for r in np.flatnonzero(self.real_s <= self.thr) if r != 50]
        assert K <= len(self.rows) < N - 8
        assert np.sort(self.dists[0][np.isfinite(self.dists[0])])[K - 1] <= self.tau

    def entries(self, rows=None):
        rows = self.rows if rows is None else rows
        beside = [50] + list(range(K))
        e = np.zeros(len(rows) + len(beside), dtype=ENT)
        for i, r in enumerate(rows):
            key = np.float32(self.real_s[r])
            e[i] = (r, self.dists[0, r], float(key) + EPS, key, 0)
        for i, r in enumerate(beside):
            e[len(rows) + i] = (r, self.dists[0, r], 0.0, 0.0, _lib.SZG_CERT_ENTRY_NO_KEY)
        return e

    def record(self, n_entries, **over):
        r = np.zeros(1, dtype=REC)
        r["query"], r["pass_"], r["keys"], r["sweep"], r["certified"], r["k"] = 0, _lib.SZG_CERT_SKETCH_TOPK_COLLECT, 0, 0, 1, K
        r["row_lo"], r["row_hi"] = 0, N
        r["thr_min"], r["kmax"] = self.tau, self.kmax
        r["thr"], r["eps"], r["D"], r["slack"] = self.thr, EPS, self.D, self.slack
        r["first_entry"], r["n_entries"] = 0, n_entries
        for k, v in over.items():
            r[k] = v
        return r

    def check(self, ents=None, eligible=None, dists=None, exc=None, **over):
        ents = self.entries() if ents is None else ents
        return cc.check(self.corpus, self.q, self.record(len(ents), **over), ents, 0, eligible=eligible,
                        dists=self.dists if dists is None else dists,
                        sketch=(self.sk_corpus, 0.0, self.exc if exc is None else exc))


@pytest.fixture(scope="module")
def world():
    return World()


def test_a_right_record_passes(world):
    s = world.check()
    assert s.records == 1 and s.checked == len(world.rows) and s.skipped == 0
    assert s.kinds == {("sketch-topk-collect", "Single", "one-sweep"): 1}
    # a query handed over before its sweep: P and R still hold on what the sample gave; no sweep on record
    none = world.entries()[:0]
    world.check(none, certified=0, thr=np.nan, eps=np.nan, D=np.nan)
    world.check(none, certified=0, thr=np.nan, eps=np.nan, D=np.nan, kmax=np.nan, thr_min=np.nan)


def test_the_pass_needs_its_inputs(world):
    ents = world.entries()
    with pytest.raises(AssertionError, match="need the sketch state"):
        cc.check(world.corpus, world.q, world.record(len(ents)), ents, 0, dists=world.dists)
    with pytest.raises(AssertionError, match="need the sketch state"):
        cc.check(world.corpus, world.q, world.record(len(ents)), ents, 0, sketch=(world.sk_corpus, 0.0, world.exc))


def test_P_can_fail(world):
    # kmax below the K-th sketched key: fewer than K rows under it (thr_min still covers what it implies: only P objects)
    keys = np.sort(np.delete(world.real_s, 50))
    with pytest.raises(AssertionError, match="P: fewer than k eligible sketched rows"):
        world.check(kmax=float(keys[K - 2] + EPS))
    # ... and rows that are not eligible do not count
    eligible = np.ones(N, dtype=bool)
    under = [r for r in np.argsort(world.real_s) if r != 50 and r >= K][:3]
    eligible[under] = False
    with pytest.raises(AssertionError, match="P: fewer than k eligible sketched rows"):
        world.check(world.entries([r for r in world.rows if r not in under]), eligible=eligible)


def test_R_can_fail(world):
    # thr_min less than the distance kmax implies plus slack (D still covers it, F still holds: only R objects)
    with pytest.raises(AssertionError, match="R: thr_min below the distance kmax implies"):
        world.check(thr_min=world.tau - 1e-6)


def test_S_k_can_fail(world):
    with pytest.raises(AssertionError, match="S_k: the sketch-distance radius does not cover"):
        world.check(D=world.tau + world.slack)   # without the factor 1 + 1e-9
    # a row outside the entries that the oracle puts within thr_min
    out = next(r for r in range(K, N) if r not in world.rows and r != 50)
    dists = world.dists.copy()
    dists[0, out] = world.tau / 2
    with pytest.raises(AssertionError, match="S_k: a row within thr_min is neither an entry nor an exception"):
        world.check(dists=dists)


def test_F_can_fail(world):
    # the oracle's K-th distance above thr_min: rows pushed away until fewer than K are within it
    dists = world.dists.copy()
    near = np.argsort(np.where(np.isfinite(dists[0]), dists[0], np.inf))
    dists[0, near[K - 1:]] = np.maximum(dists[0, near[K - 1:]], world.tau + 0.05)
    with pytest.raises(AssertionError, match="F: the k-th oracle distance is above thr_min"):
        world.check(dists=dists)
    world.check(dists=dists, certified=0)   # (handed over: nothing is claimed)
    with pytest.raises(AssertionError, match="a certified record without its sweep"):
        world.check(world.entries()[:0], thr=np.nan, eps=np.nan, D=np.nan)


def test_the_rows_beside_the_sweep(world):
    ents = world.entries()
    far = next(r for r in range(K, N) if r not in world.rows and r != 50)
    ents[-1] = (far, world.dists[0, far], 0.0, 0.0, _lib.SZG_CERT_ENTRY_NO_KEY)   # neither an exception nor a first-k row
    with pytest.raises(AssertionError, match="C_s: an entry without a key that is no exception row"):
        world.check(ents)
