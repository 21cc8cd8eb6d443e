"""The matrix sketch sweep's masked forms, host only (option sketch_masked; szg_debug_scan_masked: scan_variant's answer
for a launch with tombstones or filter masks, and the call's launches and passes as sketch_call_plan, sketch_plan_batch
and enqueue_topk split it).  Off (the default) a masked launch keeps the one-query kernel, one pass per query; on, it
takes the matrix sweep wherever the same launch without masks would: one block up to 16 queries, wide at 17 .. 32,
shared at 33 .. 64.  The tile walk of the kernels (mask_tiles.h) is checked by a stand-alone program under the address
and undefined-behaviour sanitizers (tests/cpp/test_mask_tiles.cpp, plain g++, its own main)."""
import os
import shutil
import subprocess

import pytest

from syzgydb_amd import SzgError
from syzgydb_amd.index import (option_check, scan_masked_plan, scan_matrix_plan, scan_select_plan, scan_share_plan,
                               scan_wide_plan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ((64, 0), (384, 6), (768, 12))   # dimension -> the kernel's STEPS form
FORCED = dict(sketch_wide=2, sketch_share=2)   # launches of 32 / 64 from the call's first query on (the GPU tests' setting)


def test_option_range():
    for v in (0, 1):
        option_check("sketch_masked", v)
        assert scan_masked_plan(768, 8, 16, sketch_masked=v)["serves"] == bool(v)
    for v in (-1, 2):
        with pytest.raises(SzgError, match="sketch_masked is 0 or 1"):
            option_check("sketch_masked", v)
        with pytest.raises(SzgError, match="sketch_masked is 0 or 1"):
            scan_masked_plan(768, 8, 16, sketch_masked=v)


@pytest.mark.parametrize("dim,form", FORMS)
def test_off_does_not_serve(dim, form):
    for nq in (1, 3, 16, 17, 32, 33, 40, 64, 200):
        for shared in (True, False):
            p = scan_masked_plan(dim, 8, nq, shared_mask=shared, **FORCED)
            assert not (p["serves"] or p["wide"] or p["share"] or p["tile_skip"]), (dim, nq, p)
            assert p["passes"] == nq, (dim, nq, p)   # one pass per query, as today


@pytest.mark.parametrize("dim,form", FORMS)
def test_on_serves_the_launches_the_unmasked_call_forms(dim, form):
    for kp in (1, 8, 15):
        for nq in (3, 16, 17, 32, 33, 40, 64):
            for shared in (True, False):
                p = scan_masked_plan(dim, 8, nq, kp=kp, sketch_masked=1, shared_mask=shared, **FORCED)
                what = (dim, kp, nq, shared, p)
                assert p["serves"] and p["steps"] == form, what
                assert p["wide"] == (17 <= nq <= 32) and p["share"] == (33 <= nq <= 64), what
                assert p["tile_skip"] == shared, what
                # the same launches and passes as the unmasked call of the same size
                u = scan_share_plan(dim, 8, nq, kp=kp, **FORCED)
                assert (p["launches"], p["passes"]) == (u["launches"], u["passes"]), (what, u)
    # lists of 17 .. 64 entries: one block with the serial inserts, 16 queries per pass
    for kp in (17, 64):
        p = scan_masked_plan(dim, 8, 40, kp=kp, sketch_masked=1, **FORCED)
        u = scan_share_plan(dim, 8, 40, kp=kp, **FORCED)
        assert p["serves"] and not p["wide"] and not p["share"], (dim, kp, p)
        assert (p["launches"], p["passes"]) == (u["launches"], u["passes"]) and p["passes"] < 40, (dim, kp, p, u)
    # under the automatic rules: a lone or second query keeps the one-query kernel, three take the matrix sweep
    assert not scan_masked_plan(dim, 8, 2, sketch_masked=1)["serves"]
    p = scan_masked_plan(dim, 8, 3, sketch_masked=1)
    assert p["serves"] and p["passes"] == 1, p
    p = scan_masked_plan(dim, 8, 17, sketch_masked=1)    # (a call below the wide rule: batches of 16)
    assert p["serves"] and (p["launches"], p["passes"]) == (2, 2), p
    p = scan_masked_plan(dim, 8, 1024, sketch_masked=1)  # the headline call: 16 shared launches and the edges
    u = scan_share_plan(dim, 8, 1024)
    assert (p["launches"], p["passes"]) == (u["launches"], u["passes"]) == (18, 34), (p, u)
    assert scan_masked_plan(dim, 8, 1024)["passes"] == 1024


@pytest.mark.parametrize("dim,form", FORMS)
def test_on_refuses_what_the_matrix_sweep_refuses(dim, form):
    for why, kw in (("three planes", dict(planes=3)), ("no norms", dict(norms=False)), ("untiled", dict(tiled=False)),
                    ("scan_group = 4", dict(scan_group=4)), ("kp = 96", dict(kp=96)), ("sketch_matrix = 1", dict(sketch_matrix=1))):
        for nq in (3, 16, 17, 40, 64):
            p = scan_masked_plan(dim, 8, nq, sketch_masked=1, **dict(FORCED, **kw))
            assert not (p["serves"] or p["wide"] or p["share"] or p["tile_skip"]) and p["passes"] == nq, (dim, why, nq, p)
    for bits in (4, 16, 32):
        assert not scan_masked_plan(768, bits, 16, sketch_masked=1, sketch_matrix=2)["serves"]
    # an unmasked call has no use for a masked form; its launches are the unmasked call's
    p = scan_masked_plan(dim, 8, 40, masked=False, sketch_masked=1, **FORCED)
    assert not p["serves"] and (p["launches"], p["passes"]) == (1, 2), p


@pytest.mark.parametrize("dim,form", FORMS)
def test_hooks_that_do_not_know_the_option_still_say_no(dim, form):
    for nq in (3, 16, 17, 40, 64):
        m = scan_matrix_plan(dim, 8, nq, masked=True)
        assert not m["serves"] and m["passes"] == nq, (dim, nq, m)
        assert not scan_matrix_plan(dim, 8, nq, masked=True, sketch_matrix=2)["serves"]
        assert not scan_select_plan(dim, 8, nq, masked=True)["serves"]
        assert not scan_wide_plan(dim, 8, nq, masked=True, sketch_wide=2)["serves"]
        assert not scan_share_plan(dim, 8, nq, masked=True, **FORCED)["serves"]


def test_standalone_mask_tiles_program_is_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_mask_tiles.cpp"
    exe = str(tmp_path / "test_mask_tiles")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_mask_tiles.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "mask tiles ok" in done.stdout
