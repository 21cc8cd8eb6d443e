"""Keys at and near zero, host only: the planted inputs of tests/test_gpu_coincident.py stand where they claim to stand
(the oracle and cert_check.Corpus alone, no library call), the certification bound as a unit (csrc/key_bound.h) under
the address and undefined-behaviour sanitizers (tests/cpp/test_key_bound.cpp, plain g++, its own main), and the
library's hook szg_debug_key_eps against the bounds that program prints."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import coincident_cases as cases
import oracle as orc
from syzgydb_amd import SzgError
from syzgydb_amd.index import key_eps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_NAMES = {0: "one-sweep", 1: "int8", 2: "bf16", 3: "f32"}

# (bits, dim, queries, largest |Q| of the path, far): one of every width and every spacing rule the GPU file uses
PLANTED = [(32, 43, 8, None, False), (32, 43, 8, None, True), (64, 24, 16, None, False), (64, 24, 16, None, True),
           (16, 87, 8, None, False), (16, 17, 16, None, False), (8, 175, 8, cases.QMAX_ONE_SWEEP[8], False),
           (8, 192, 64, cases.QMAX_SHARED, False), (4, 351, 8, cases.QMAX_ONE_SWEEP[4], False),
           (4, 200, 16, cases.QMAX_SHARED, False), (32, 64, 136, None, False), (32, 100, 32, None, False),
           (32, 40, 16, None, True), (64, 24, 16, None, True), (32, 64, 136, None, True)]


@pytest.mark.parametrize("bits,dim,nq,qmax,far", PLANTED, ids=["%db-d%d-q%d%s" % (b, d, q, "-far" if f else "") for b, d, q, _, f in PLANTED])
def test_planted_inputs_stand_where_they_claim(bits, dim, nq, qmax, far):
    case = cases.build(bits, dim, nq, 0, qmax=qmax, far=far)
    c = case.corpus
    assert c.n % 16 == 5 and nq * c.n * dim <= cases.cc.WIDE_LIMIT
    assert (c.packed[list(case.copies)] == c.packed[case.r0]).all()
    assert case.copies[0] < 16 and c.n - case.copies[2] <= 5 and 16 < case.copies[1] < c.n - 16
    zero_rows = sorted(case.copies + (case.r0,))
    for metric in (0, 1):
        m = case.with_metric(metric)
        real, err = m.corpus.keys(m.Q)
        for qi, row, kind in m.planted:
            # the planted row has the smallest real-number key (P0: together with its copies)
            order = np.argsort(real[qi], kind="stable")
            first = zero_rows if kind == "P0" else [row]
            assert sorted(int(x) for x in order[: len(first)]) == first, (metric, qi, kind, order[:5])
            off = real[qi] + metric   # (a cosine key is -cos: 0 at the planted row after + 1)
            assert off[order[len(first)]] > 100 * max(off[row], 0) + 1e-9, "the next row is nowhere near"
            if metric == 0:
                got_rows, got_dist, _ = orc.search_exact(c.packed, dim, bits, 0, m.Q[qi], k=len(first))
                assert sorted(int(x) for x in got_rows) == first, (qi, kind, got_rows)
                if kind == "P0":
                    assert real[qi, row] == 0.0 and (got_dist == 0.0).all(), (real[qi, row], got_dist)
                else:
                    assert real[qi, row] > 0.0 and got_dist[0] > 0.0, (qi, kind, real[qi, row], got_dist)
    if bits in (16, 32):
        # P1 stands on the gap: every float32 difference of the one-sweep kernel is 0, the real-number key is not
        real, _ = case.corpus.keys(case.Q)
        qi, row, kind = case.planted[1]
        assert kind == "P1" and cases.float32_key(case, qi, row) == 0.0 and real[qi, row] > 0.0
        assert cases.float32_key(case, 0, case.r0) == 0.0
        for qi, row, kind in case.planted[2:]:
            assert cases.float32_key(case, qi, row) > 0.0, (qi, kind)


def test_parallel_queries_of_the_cosine_leg():
    case = cases.build_parallel(32, 40, 16)
    d = case.dists()
    for qi, row, kind in case.planted:
        assert np.nanargmin(d[qi]) == row or np.isnan(d[qi, row]), (qi, kind, d[qi, row])
        assert np.isnan(d[qi, row]) or d[qi, row] < 1e-6


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_key_bound.cpp"
    exe = str(tmp_path_factory.mktemp("key_bound") / "test_key_bound")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_key_bound.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-4000:] + done.stderr[-4000:]
    return done.stdout


def test_standalone_key_bound_program_is_clean_under_sanitizers(program_output):
    assert "key bound ok" in program_output
    assert "the formula without the query term fails" in program_output


def test_hook_agrees_with_the_header(program_output):
    lines = [ln.split() for ln in program_output.splitlines() if ln.startswith("BOUND ")]
    assert len(lines) >= 50
    families = set()
    for f in lines:
        dim, bits, metric, planes, mq_planes, family = (int(x) for x in f[1:7])
        key, qnorm, qnorm2, qscale, mq_qscale = (float.fromhex(x) for x in f[7:12])
        want = float.fromhex(f[13])
        got = key_eps(dim, bits, metric, key, qnorm, qnorm2, family=FAMILY_NAMES[family], planes=planes, qscale=qscale,
                      mq_qscale=mq_qscale, mq_planes=mq_planes)
        assert got == want, (f, got.hex())
        families.add((family, bits, metric))
    assert {x[0] for x in families} == {0, 1, 2, 3}


def test_float_row_bound_at_a_zero_key():
    u = 2.0 ** -24
    for bits, dim, qnorm in ((32, 768, 27.7), (16, 17, 1.5e5), (32, 3, 1e-3)):
        at0 = key_eps(dim, bits, 0, 0.0, qnorm, qnorm * qnorm)
        assert at0 >= u * u * qnorm * qnorm   # what the narrowing of the query can leave under a float32 key of 0
        assert at0 <= 16.0 * u * u * qnorm * qnorm + 1e-30   # ... and no more than a small multiple of it
        # at a key of the size of |g|^2 the term is below a 10^-6 of the bound
        k = qnorm * qnorm
        assert 4.0 * u * u * k < 1e-6 * key_eps(dim, bits, 0, k, qnorm, k)
    assert key_eps(24, 64, 0, 0.0, 1e3, 1e6) >= 2.0 ** -149   # 64-bit rows: the narrowing of the key to float32
    for bad in (dict(dim=0), dict(quant_bits=5), dict(metric=2), dict(planes=4)):
        a = dict(dict(dim=8, quant_bits=32, metric=0, key=0.0, qnorm=1.0, qnorm2=1.0), **bad)
        with pytest.raises(SzgError):
            key_eps(**a)
    with pytest.raises(SzgError, match="8- and 4-bit"):
        key_eps(8, 32, 0, 0.0, 1.0, 1.0, family="int8")
