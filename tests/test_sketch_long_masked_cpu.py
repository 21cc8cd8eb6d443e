"""The masked long-row forms of the matrix sketch sweep, host only (szg_debug_scan_long_masked, szg_debug_scan_masked):
under sketch_masked = 1 a launch with tombstones or filter masks takes the long form exactly where the unmasked launch
of the same size does, with its blocks, threads, grid, LDS and passes; under 0 it keeps the one-query kernel."""
import pytest

from syzgydb_amd.index import scan_long_plan, scan_masked_plan, scan_share_plan

KEYS = ("serves", "blocks", "share", "block", "grid", "lds_bytes", "passes")
# Column blocks (2: wide and shared) whose masked instantiation was left out for want of registers -- launches of 16 instead:
LEFT_OUT = ()   # none: the wide kernels take 247 / 255 VGPRs, the shared ones 223 / 231, no scratch


@pytest.mark.parametrize("kp", (8, 12, 24))
def test_masked_launch_takes_the_unmasked_launch_s_plan(kp):
    for dim in range(1024, 4096 + 64, 64):
        short = 16 * (2 * dim + 12 + 8 * 4 * kp) <= 64 * 1024   # the one-block form of 64 KiB serves the shape
        for nq in (16, 32, 64):
            u = scan_long_plan(dim, 8, nq, kp=kp)
            assert u["serves"] == (not short) and u["blocks"] not in LEFT_OUT, (dim, kp, nq, u)
            for shared in (True, False):
                m = scan_long_plan(dim, 8, nq, kp=kp, masked=True, sketch_masked=1, shared_mask=shared)
                assert {x: m[x] for x in KEYS} == {x: u[x] for x in KEYS}, (dim, kp, nq, m, u)
                assert m["tile_skip"] == (shared and u["serves"]), (dim, kp, nq, shared, m)
                off = scan_long_plan(dim, 8, nq, kp=kp, masked=True, sketch_masked=0, shared_mask=shared)
                assert not off["serves"] and not off["tile_skip"] and off == scan_long_plan(dim, 8, nq, kp=kp, masked=True), (dim, off)
            assert {x: scan_long_plan(dim, 8, nq, kp=kp, sketch_masked=1)[x] for x in KEYS} == {x: u[x] for x in KEYS}
        assert not short or scan_masked_plan(dim, 8, 16, kp=kp, sketch_masked=1)["serves"], (dim, kp)   # (the 64 KiB masked form)


@pytest.mark.parametrize("dim", (2048, 4096))
def test_a_masked_call_splits_as_the_unmasked_call(dim):
    for nq in (3, 21, 1024):
        for shared in (True, False):
            p = scan_masked_plan(dim, 8, nq, sketch_masked=1, shared_mask=shared)
            u = scan_share_plan(dim, 8, nq)
            assert (p["launches"], p["passes"]) == (u["launches"], u["passes"]) and p["passes"] < nq, (dim, nq, p, u)
            assert scan_masked_plan(dim, 8, nq, sketch_masked=0, shared_mask=shared)["passes"] == nq, (dim, nq)
