"""The matrix sketch sweep's shared form, host only (szg_debug_scan_share: scan_variant's answer under option
sketch_share, and the call's batches as sketch_call_plan / sketch_plan_batch split it).  A launch of 33 to 64 queries is
one shared launch -- two column groups of 32 on paired blocks, two passes over the rows -- exactly where the two-block
form would serve 32 of them.  The automatic rule starts at 136 queries (2 x 64 + 2 x 4); shorter calls keep their plan.
The hook's shape is the hooks' 4M rows on 256 CUs: a plain grid of 512 blocks, so S = 256 slices."""
import pytest

from syzgydb_amd import SzgError
from syzgydb_amd.index import scan_matrix_plan, scan_wide_plan, scan_share_plan, option_check

DIMS = (64, 384, 768)
WAVES = 4
# the wide hook's refusals (tests/test_sketch_wide_cpu.py)
NOT_SERVED = (("masked", dict(masked=True)), ("three planes", dict(planes=3)), ("untiled", dict(tiled=False)),
              ("no norms", dict(norms=False)), ("kp = 17", dict(kp=17)), ("kp = 64", dict(kp=64)),
              ("scan_group = 1", dict(scan_group=1)), ("scan_group = 2", dict(scan_group=2)),
              ("scan_group = 4", dict(scan_group=4)), ("sketch_matrix = 1", dict(sketch_matrix=1)),
              ("sketch_select = 1", dict(sketch_select=1)), ("sketch_wide = 1", dict(sketch_wide=1)))


def lds_bytes(dim, kp, blocks):
    dim64 = (dim + 63) // 64 * 64
    return 16 * blocks * (2 * dim64 + 12 + 8 * WAVES * kp)


def test_option_range():
    for v in (0, 1, 2):
        option_check("sketch_share", v)
        option_check("sketch_wide", v)
    for v in (-1, 3, 4):
        with pytest.raises(SzgError):
            option_check("sketch_share", v)
        with pytest.raises(SzgError):
            option_check("sketch_wide", v)
        with pytest.raises(SzgError):
            scan_share_plan(768, 8, 64, sketch_share=v)


@pytest.mark.parametrize("dim", DIMS)
def test_serves_launches_of_33_to_64(dim):
    for kp in (1, 8, 15):
        for nq in (33, 48, 63, 64):
            for share in (0, 2):
                p = scan_share_plan(dim, 8, nq, kp=kp, sketch_share=share)
                what = (dim, kp, nq, share, p)
                assert p["serves"] and p["slices"] == 256, what
                assert p["lds_bytes"] == lds_bytes(dim, kp, 2) <= 64 * 1024, what
        for nq in (1, 16, 17, 32):   # fewer than 33 queries: no shared launch
            p = scan_share_plan(dim, 8, nq, kp=kp, sketch_share=2)
            assert not p["serves"] and p["slices"] == 0, (dim, kp, nq, p)
        assert not scan_share_plan(dim, 8, 64, kp=kp, sketch_share=1)["serves"]
    # 768 dimensions with lists of 16: two blocks do not fit 64 KiB
    assert scan_share_plan(dim, 8, 64, kp=16, sketch_share=2)["serves"] == (lds_bytes(dim, 16, 2) <= 64 * 1024)


@pytest.mark.parametrize("dim", DIMS)
def test_does_not_serve(dim):
    for nq in (33, 64, 200):
        for why, kw in NOT_SERVED:
            kw = dict(dict(kp=8), **kw)
            for share in (0, 2):
                p = scan_share_plan(dim, 8, nq, **dict(dict(sketch_share=share), **kw))
                assert not p["serves"] and p["slices"] == 0, (dim, nq, why, p)
                assert max(p["batches"]) <= 32, (dim, nq, why, p)   # no batch needs a shared launch
                assert sum(p["batches"]) == nq
    for dim_ in (48, 100):
        assert not scan_share_plan(dim_, 8, 64, sketch_matrix=2, sketch_share=2)["serves"]
    for bits in (4, 16, 32):
        assert not scan_share_plan(768, bits, 64, sketch_matrix=2, sketch_share=2)["serves"]


def test_batches_of_the_automatic_rule():
    p = scan_share_plan(768, 8, 135)   # below the threshold: today's wide plan
    assert p["batches"] == [4, 32, 32, 32, 31, 4] and p["launches"] == 6 and p["passes"] == 6
    p = scan_share_plan(768, 8, 136)
    assert p["batches"] == [4, 64, 64, 4] and p["launches"] == 4 and p["passes"] == 6
    p = scan_share_plan(768, 8, 200)
    assert p["batches"] == [4, 64, 64, 64, 4] and p["launches"] == 5 and p["passes"] == 8
    p = scan_share_plan(768, 8, 1024)
    assert p["batches"] == [4] + [64] * 15 + [56, 4] and p["launches"] == 18 and p["passes"] == 34
    p = scan_share_plan(768, 8, 100)   # (tests/test_gpu_sketch_wide.py pins this plan)
    assert p["batches"] == [4, 32, 32, 28, 4]
    p = scan_share_plan(768, 8, 71)    # below the wide threshold too: batches of 16
    assert p["batches"] == [4, 16, 16, 16, 15, 4]
    # never: the wide plan at every length
    assert scan_share_plan(768, 8, 1024, sketch_share=1)["batches"] == [4] + [32] * 31 + [24, 4]
    assert scan_share_plan(768, 8, 1024, sketch_wide=1)["batches"] == [4] + [16] * 63 + [8, 4]


def test_batches_when_forced():
    for nq, want, launches, passes in ((33, [33], 1, 2), (64, [64], 1, 2), (65, [64, 1], 2, 3), (96, [64, 32], 2, 3),
                                       (97, [64, 33], 2, 4), (136, [64, 64, 8], 3, 5), (32, [32], 3, 3)):
        # (32: not a share call but a short one under the default plan -- one batch whose sweeps launch in two parts, 28
        # queries as 16 + 12 and then the last 4: the hook counts the launches the call makes, sketch_plan.h's)
        p = scan_share_plan(768, 8, nq, sketch_share=2)
        assert (p["batches"], p["launches"], p["passes"]) == (want, launches, passes), (nq, p)


@pytest.mark.parametrize("dim", DIMS)
def test_the_wide_and_matrix_hooks_answer_as_before(dim):
    for nq in (3, 16, 17, 32, 33, 40, 48, 64, 96):
        for kp in (1, 8, 16, 17, 64):
            m = scan_matrix_plan(dim, 8, nq, kp=kp)
            assert m["serves"] and m["passes"] == -(-nq // 16), (dim, nq, kp, m)
            assert m["lds_bytes"] == lds_bytes(dim, kp, 1), (dim, nq, kp, m)
        for kp in (1, 8):
            for wide in (0, 2):
                w = scan_wide_plan(dim, 8, nq, kp=kp, sketch_wide=wide)
                assert w["serves"] == (nq > 16) and w["passes"] == -(-nq // 32), (dim, nq, kp, wide, w)
                assert w["lds_bytes"] == lds_bytes(dim, kp, 2 if nq > 16 else 1), (dim, nq, kp, wide, w)
