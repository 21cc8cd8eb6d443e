"""The plans of the long-row collect form (16 b (2 dim + 16) bytes of LDS) and the long sample pass (b (2 KiB steps + 192))
against their formulas; the 64 KiB forms' hooks answer as before."""
import pytest

from syzgydb_amd.index import sample_long_plan, sample_plan, scan_collect_plan, scan_long_collect_plan, scan_plan

DIMS = (1024, 1984, 2048, 2496, 2560, 3072, 4096)


@pytest.mark.parametrize("dim", DIMS + (4160,))
def test_collect_plan(dim):
    grid = scan_plan(dim, 8, 1 << 22, kp=0)["grid"]
    for nq in (3, 16, 19, 32):
        p = scan_long_collect_plan(dim, 8, nq)
        if dim < 2048 or dim > 4096:   # (the 64 KiB forms' rows, and 65 steps: one more than the long stream walks)
            assert not p["serves"] and p["block"] == 256 and p["grid"] == grid, (dim, nq, p)
            continue
        two = nq > 16 and 32 * (2 * dim + 16) <= 160 * 1024
        big = two or 16 * (2 * dim + 16) > 80 * 1024
        want = {"serves": True, "blocks": 2 if two else 1, "block": 512 if big else 256, "grid": (grid + 1) // 2 if big else grid,
                "passes": 1 if two or nq <= 16 else 2, "lds_bytes": (32 if two else 16) * (2 * dim + 16)}
        assert p == want, (dim, nq, p, want)
    if 2048 <= dim <= 4096:
        assert scan_long_collect_plan(dim, 8, 32, sketch_wide=1)["blocks"] == 1
        assert scan_long_collect_plan(dim, 8, 2) == dict(scan_long_collect_plan(dim, 8, 2), serves=False, passes=2)
        for off in ({"masked": True}, {"planes": 3}, {"tiled": False}, {"norms": False}):
            p = scan_long_collect_plan(dim, 8, 16, **off)
            assert not p["serves"] and p["passes"] == 16 and p["block"] == 256, (dim, off, p)
        assert not scan_long_collect_plan(dim, 32, 16)["serves"]


@pytest.mark.parametrize("dim", DIMS)
def test_sample_plan(dim):
    rows, k, steps = 200000, 100, dim // 64
    for nq in (1, 16, 17, 32):
        p = sample_long_plan(rows, k, nq, dim, cu_count=256)
        if dim < 2048:
            assert p == dict.fromkeys(p, 0) and not p["serves"], (dim, nq, p)
            continue
        two = nq > 16 and 2 * (2048 * steps + 192) <= 160 * 1024
        lds = (2 if two else 1) * (2048 * steps + 192)
        big, tiles = two or lds > 80 * 1024, -(-(-(-rows // 16)) // p["stride"])
        assert p["serves"] and p["blocks"] == (2 if two else 1) and p["block"] == (512 if big else 256) and p["lds_bytes"] == lds, (dim, nq, p)
        assert p["tiles"] == tiles and p["slots"] == 16 * tiles and p["grid"] == min(-(-tiles // (8 if big else 4)), 256 * (1 if big else 2)), (dim, nq, p)
    assert not sample_long_plan(rows, 4000, 1, dim)["serves"] and not sample_long_plan(rows, k, 1, dim, planes=3)["serves"]


@pytest.mark.parametrize("dim", (1024, 2048, 4096))
def test_the_hooks_of_the_64_kib_forms_answer_as_before(dim):
    for nq, wide in ((16, 0), (32, 2)):
        p = scan_collect_plan(dim, 8, nq, sketch_wide=wide)
        assert p["serves"] == (dim == 1024) and p["lds_bytes"] <= 64 * 1024 and p["passes"] == (nq // 16 if dim == 1024 else nq), (dim, p)
    assert sample_plan(200000, 100, 1, dim)["serves"] == (dim == 1024)
