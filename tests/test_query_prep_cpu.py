"""The rule by which a query becomes the 8-bit sweep's image and constants (syzgydb_amd/csrc/query_prep.h), which the
host form and the kernel of option query_prep both follow, against the rule restated in Python (query_prep_cases.prepare:
not a line of the header): image bytes and the float64 bit patterns of qnorm, m1, qscale, qconst, qnorm2 -- for both
metrics, two and three digit planes, a Euclidean sketch scale, dimensions with a partial 16-element piece and partial
plane words, and the vectors the rule can go wrong on (zero, NaN, +-Inf, equal elements, signed zeros and subnormals, an
overflowing m1, a single element, ties of the rounding on both signs, every borrow of the balanced digit split).  And the
batch rule of the option (sketch_plan.h: query_prep_serves, kQueryPrepMin).  A stand-alone program
(tests/cpp/test_query_prep.cpp, plain g++, its own main) runs under the address and undefined-behaviour sanitizers; no
GPU, no library load."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import query_prep_cases as qpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (1, 15, 16, 17, 64, 100, 384, 768)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_query_prep.cpp"
    out = str(tmp_path_factory.mktemp("query_prep") / "test_query_prep")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", out, os.path.join(ROOT, "tests", "cpp", "test_query_prep.cpp"),
                    os.path.join(ROOT, "syzgydb_amd", "csrc", "scan_plan.cpp")], check=True)
    return out


def run(exe, tmp_path, Q, cosine, planes, gs):
    path = str(tmp_path / "q.bin")
    np.ascontiguousarray(Q, dtype="<f8").tofile(path)
    done = subprocess.run([exe, path, str(Q.shape[1]), str(Q.shape[0]), str(cosine), str(planes), repr(float(gs))],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert "query prep ok" in done.stdout
    return done.stdout.splitlines()


@pytest.mark.parametrize("planes", (2, 3))
@pytest.mark.parametrize("cosine", (1, 0), ids=["cos", "euc"])
def test_header_follows_the_restated_rule(exe, tmp_path, cosine, planes):
    for dim in DIMS:
        for gs in ((0.0,) if cosine else (0.0, 3.7)):
            vecs = qpc.vectors(dim, planes, 77 + dim)
            Q = np.stack(list(vecs.values()))
            lines = run(exe, tmp_path, Q, cosine, planes, gs)
            images = [ln.split()[1] for ln in lines if ln.startswith("image ")]
            metas = [[int(x, 16) for x in ln.split()[1:]] for ln in lines if ln.startswith("meta ")]
            assert len(images) == len(metas) == len(vecs)
            for j, name in enumerate(vecs):
                what = (name, "dim", dim, "cosine", cosine, "planes", planes, "gs", gs)
                image, meta = qpc.prepare(Q[j], cosine, planes, gs)
                assert len(image) == 48 * ((dim + 15) // 16)
                assert images[j] == image.hex(), ("image", what)
                assert metas[j] == [qpc.bits(x) for x in meta], ("constants", what, metas[j], meta)


def test_the_vectors_reach_what_they_are_for():
    """The special vectors do what their names say under the restated rule -- so a pass above means something."""
    dim = 64
    for planes, qmax in ((2, 16000), (3, 1000000)):
        vecs = qpc.vectors(dim, planes, 5)

        def Qs(name, cosine):
            image, meta = qpc.prepare(vecs[name], cosine, planes)
            r16 = dim // 16
            out = []
            for e in range(dim):
                val = 0
                for x in range(3 - planes, 3):
                    b = image[((x * r16 + e // 16) * 4 + (e % 16) // 4) * 4 + (e % 16) % 4]
                    val = val * 128 + (b - 256 if b >= 128 else b)
                out.append(val)
            return out, meta

        q, meta = Qs("zero", 1)
        assert set(q) == {0} and meta[2] == 1.0 and meta[1] == 0.0          # cosine scale 0, qs = 1
        q, meta = Qs("pos_inf", 0)
        assert meta[2] == 1.0 and q[dim - 1] == qmax                          # vmax not finite: qs = 1, the clamp
        q, meta = Qs("pos_inf", 1)
        assert np.isnan(meta[0]) and np.isnan(meta[4]) and np.isinf(meta[1])  # inf * 0 on the way to qnorm2
        q, meta = Qs("nan", 1)
        assert np.isnan(meta[1]) and meta[2] == 1.0 and set(q) == {0}
        q, meta = Qs("huge", 0)
        assert np.isinf(meta[1])                                              # m1 overflows
        q, meta = Qs("single_nonzero", 1)
        assert sorted(set(q)) == [0, qmax]
        q, meta = Qs("single_negative", 0)
        assert sorted(set(q)) == [-qmax, 0]
        q, meta = Qs("ties", 0)
        assert meta[2] == 255.0 and q[0] == qmax
        # the ties themselves go away from zero, not to even: 0.5 -> 1, -0.5 -> -1, 2.5 -> 3, -2.5 -> -3, 8191.5 -> 8192,
        # -8192.5 -> -8193 (their neighbours in the last place go where t + 1/2 rounds: the restated rule says)
        assert [q[i] for i in (1, 4, 13, 16, 43, 46)] == [1, -1, 3, -3, 8192, -8193], q[:48]
        assert q[14] in (2, 3) and q[15] == 3 and q[17] in (-2, -3) and q[18] == -3, q[:20]
        q, meta = Qs("digit_borrow", 0)
        assert meta[2] == 255.0 and q[0] == -qmax
        want = [v for v in qpc._DIGITS if abs(v) <= qmax]
        assert q[1:1 + len(want)] == want


def test_batch_rule(exe, tmp_path):
    lines = run(exe, tmp_path, np.zeros((0, 4)), 1, 2, 0.0)
    least = [int(ln.split()[1]) for ln in lines if ln.startswith("min ")]
    assert len(least) == 1 and 2 <= least[0] <= 32, least   # (a lone search and the 4-query edges stay on the host)
    seen = {}
    for ln in lines:
        if ln.startswith("serves "):
            o, b, s = (int(x) for x in ln.split()[1:])
            seen[o, b] = s
    assert len(seen) == 5 * 71
    for (o, b), s in seen.items():
        want = b >= 1 and (o == 2 or (o == 1 and b >= least[0]))
        assert s == int(want), (o, b, s)
