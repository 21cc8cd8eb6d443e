"""The arithmetic every certificate of a call through the 8-bit sketch rests on (syzgydb_amd/csrc/sketch_bound.h: slack, the
two conversions between a key bound and a sketch distance, the certificate's predicate, the collect radius, the queries and
radii that are handed over, the scaled query), which the three sketch pipelines share, against the rules restated here with
math.acos and math.sqrt -- not a line of the header -- bit for bit: both metrics, Euclidean scales down to 1e-150 and up to
1e200, keys at, beside and beyond the ends of a cosine's range, zero of both signs, the largest float32, Inf and NaN.  The
slack also against cert_check.sketch_slack, which the GPU checks use.  A stand-alone program (tests/cpp/test_sketch_bound.cpp,
plain g++, its own main) runs under the address and undefined-behaviour sanitizers and itself holds the two conversions to a
long double reference of the real formulas (below <= exact <= above, monotone, within their constants, nothing finite from an
overflow); no GPU, no library load."""
import math
import os
import shutil
import struct
import subprocess

import pytest

from syzgydb_amd import cert_check as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
KEYS = (-2.0, -1.0 - 1e-15, -1.0, -1.0 + 1e-16, -0.5, -1e-300, -0.0, 0.0, 1e-300, 0.5, 1.0 - 1e-16, 1.0, 1.0 + 1e-15, 2.0,
        3e38, INF, NAN)
SCALES = (0.0, 3.7, 1e-150, 1e200)   # 0: cosine
DIMS = (1, 222, 223, 768, 4096)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def val(token):
    return struct.unpack("<d", struct.pack("<Q", int(token, 16)))[0]


def same(token, want):
    """Equal bits; a NaN for a NaN (its sign and payload are the compiler's and the libm's, and mean nothing)."""
    return math.isnan(val(token)) if math.isnan(want) else int(token, 16) == bits(want)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_sketch_bound.cpp"
    out = str(tmp_path_factory.mktemp("sketch_bound") / "test_sketch_bound")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", out, os.path.join(ROOT, "tests", "cpp", "test_sketch_bound.cpp")], check=True)
    done = subprocess.run([out], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-4000:] + done.stderr[-4000:]   # (its own assertions, and the sanitizers)
    assert "sketch bound ok" in done.stdout
    return [ln.split() for ln in done.stdout.splitlines()]


def of(lines, word):
    return [ln[1:] for ln in lines if ln[0] == word]


# ---- the rules, restated ------------------------------------------------------------------------------------------------

def slack(max_ang, gs, dim):
    rounding = 0.0
    if not gs > 0.0:
        rounding = max(1e-7, 2.0 * math.sqrt((dim + 8) * 2.0 ** -52) / math.pi)
    return max_ang * (1.0 + 1e-9) + rounding


def distance(gs, key, up):
    """The sketch distance a key bound implies, every rounding pushed up (an upper bound) or down (a lower one)."""
    if gs > 0.0:
        root = math.sqrt(0.0 if key < 0.0 else key)
        return gs * root / 255.0 * ((1.0 + 1e-9) if up else (1.0 - 1e-9))
    cosine = (-key - 1e-15) if up else (-key + 1e-15)
    if cosine >= 1.0:
        return 0.0
    if cosine <= -1.0:
        return 1.0
    return math.acos(cosine) / math.pi * ((1.0 + 1e-12) if up else (1.0 - 1e-12))


def settles(kth, d_lb, slk):
    return math.isfinite(d_lb) and kth * (1.0 + 1e-9) < d_lb - slk


def collect_radius(r, slk):
    return r * (1.0 + 1e-9) + slk


def radius_handed(gs, d):
    return not math.isfinite(d) or (not gs > 0.0 and d >= 1.0)


def query_handed(q, gs):
    total = 0.0
    for x in q:
        if not math.isfinite(x):
            return True
        total += x * x
    return not math.isfinite(total) or (not gs > 0.0 and total == 0.0)


# ---- the header against them ------------------------------------------------------------------------------------------------

def test_slack(lines):
    seen = set()
    for ang, gs, dim, got in of(lines, "slack"):
        ang, gs, dim = val(ang), val(gs), int(dim)
        assert same(got, slack(ang, gs, dim)), (ang, gs, dim)
        assert same(got, cc.sketch_slack(ang, gs, dim)), ("cert_check.sketch_slack", ang, gs, dim)
        seen.add((gs > 0.0, dim))
    assert seen == {(e, d) for e in (False, True) for d in DIMS}


@pytest.mark.parametrize("word", ("below", "above"))
def test_key_bound_to_distance(lines, word):
    seen = {}
    for gs, key, got in of(lines, word):
        gs, key = val(gs), val(key)
        want = distance(gs, key, word == "above")
        assert same(got, want), (word, gs, key, val(got), want)
        seen.setdefault(bits(gs), set()).add(bits(key))
    assert set(seen) == {bits(g) for g in SCALES}
    for g in SCALES:
        assert seen[bits(g)] >= {bits(k) for k in KEYS}, g


def test_certificate_and_radius(lines):
    rows = of(lines, "settles")
    assert len(rows) >= 100
    for kth, d, slk, got in rows:
        assert int(got) == int(settles(val(kth), val(d), val(slk))), (val(kth), val(d), val(slk))
    radii = {}
    for r, slk, got in of(lines, "radius"):
        assert same(got, collect_radius(val(r), val(slk))), (val(r), val(slk))
        radii.setdefault(bits(val(r)), []).append(int(got, 16))
    assert set(radii) >= {bits(r) for r in (0.0, 0.5, 1.0, INF, NAN)}
    for gs, d, got in of(lines, "keyradius"):
        gs, d = val(gs), val(d)
        assert same(got, d / gs if gs > 0.0 else d), (gs, d)
    handed = {}
    for gs, d, got in of(lines, "rhanded"):
        assert int(got) == int(radius_handed(val(gs), val(d))), (val(gs), val(d))
        handed[bits(val(gs)), int(d, 16)] = int(got)
    # under cosine: the collect radius of each radius of the list, at each slack, was asked -- R = 1 and beyond, Inf and NaN
    # are handed over, R = 0 and 0.5 at these slacks are not
    for r, want in ((0.0, 0), (0.5, 0), (1.0, 1), (INF, 1), (NAN, 1)):
        for d in radii[bits(r)]:
            assert handed[bits(0.0), d] == want, (r, d)
    assert handed[bits(3.7), bits(1.5)] == 0 and handed[bits(0.0), bits(1.5)] == 1   # (D >= 1 means nothing under Euclid)


def test_queries(lines):
    queries = {ln[0]: [val(t) for t in ln[1:]] for ln in of(lines, "query")}
    assert set(queries) >= {"plain", "nan_first", "nan_last", "inf_first", "inf_last", "zero", "squares_overflow"}
    assert math.isnan(queries["nan_first"][0]) and math.isnan(queries["nan_last"][-1])
    assert math.isinf(queries["inf_first"][0]) and math.isinf(queries["inf_last"][-1])
    assert all(math.isfinite(x) for x in queries["squares_overflow"]) and query_handed(queries["squares_overflow"], 3.7)
    seen = set()
    for name, gs, got in of(lines, "qhanded"):
        gs = val(gs)
        assert int(got) == int(query_handed(queries[name], gs)), (name, gs)
        seen.add((name, gs > 0.0))
        if name == "plain":
            assert int(got) == 0
        if name in ("zero", "negative_zero", "squares_underflow"):
            assert int(got) == (0 if gs > 0.0 else 1), (name, gs)      # no direction: cosine alone hands it over
    assert seen == {(n, e) for n in queries for e in (False, True)}
    n = 0
    for ln in of(lines, "scaled"):
        name, gs, got = ln[0], val(ln[1]), ln[2:]
        want = [x / gs if gs > 0.0 else x for x in queries[name]]
        assert len(got) == len(want) and all(same(g, w) for g, w in zip(got, want)), (name, gs)
        n += 1
    assert n == len(queries) * len(SCALES)
