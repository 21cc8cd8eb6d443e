"""The matrix sketch sweep's two-block form, host only (szg_debug_scan_wide: scan_variant's answer under option
sketch_wide): a launch of 17 to 32 queries scores 32 queries per row read exactly where the matrix sweep serves it with
row lists -- tiled two-plane 8-bit rows of whole 64-byte steps with resident norms, lists of at most 16 entries -- and
both column blocks fit 64 KiB of LDS.  Documented LDS (include/syzgy_scan.h): with b column blocks,
16 b (2 dim64 + 12 + 8 waves kp) bytes, dim64 = the row bytes in whole 64-byte steps, waves = 4.  768 dimensions with
lists of 16 would need 65 920 bytes: such launches keep one block.  What szg_debug_scan_matrix reports does not change."""
import pytest

from syzgydb_amd import SzgError
from syzgydb_amd.index import scan_matrix_plan, scan_wide_plan, option_check

DIMS = (64, 384, 768)
COUNTS = (16, 17, 31, 32, 33, 48, 96)
KPS = (1, 8, 16)
WAVES = 4
NOT_SERVED = (("masked", dict(masked=True)), ("three planes", dict(planes=3)), ("untiled", dict(tiled=False)),
              ("no norms", dict(norms=False)), ("kp = 17", dict(kp=17)), ("kp = 64", dict(kp=64)),
              ("scan_group = 1", dict(scan_group=1)), ("scan_group = 2", dict(scan_group=2)),
              ("scan_group = 4", dict(scan_group=4)), ("sketch_matrix = 1", dict(sketch_matrix=1)),
              ("sketch_select = 1", dict(sketch_select=1)), ("sketch_wide = 1", dict(sketch_wide=1)))


def lds_bytes(dim, kp, blocks):
    dim64 = (dim + 63) // 64 * 64
    return 16 * blocks * (2 * dim64 + 12 + 8 * WAVES * kp)


def fits(dim, kp):
    return lds_bytes(dim, kp, 2) <= 64 * 1024


def test_the_formula_at_the_headline_shape():
    assert lds_bytes(768, 8, 2) == 57728 and lds_bytes(768, 16, 2) == 65920
    assert fits(768, 15) and not fits(768, 16)
    assert all(fits(dim, kp) for dim in (64, 384) for kp in KPS)


@pytest.mark.parametrize("dim", DIMS)
def test_serves_row_list_launches_of_more_than_16(dim):
    for kp in KPS:
        for nq in COUNTS:
            for wide in (0, 2):
                p = scan_wide_plan(dim, 8, nq, kp=kp, sketch_wide=wide)
                what = (dim, kp, nq, wide, p)
                if fits(dim, kp):
                    assert p["serves"] == (nq > 16), what
                    assert p["passes"] == -(-nq // 32), what
                    assert p["lds_bytes"] == lds_bytes(dim, kp, 2 if nq > 16 else 1), what
                else:   # one block: launches of 16
                    assert not p["serves"] and p["passes"] == -(-nq // 16), what
                    assert p["lds_bytes"] == lds_bytes(dim, kp, 1), what
                assert p["lds_bytes"] <= 64 * 1024, what


@pytest.mark.parametrize("dim", DIMS)
def test_does_not_serve(dim):
    for nq in COUNTS:
        for why, kw in NOT_SERVED:
            kw = dict(dict(kp=8), **kw)
            for wide in (0, 2):
                if "sketch_wide" in kw and wide == 2:
                    continue
                p = scan_wide_plan(dim, 8, nq, **dict(dict(sketch_wide=wide), **kw))
                assert not p["serves"], (dim, nq, why, p)
                assert p["lds_bytes"] <= 64 * 1024, (dim, nq, why, p)
    # the launches it does not serve are launches of up to 16: what the matrix hook says of them
    for nq in COUNTS:
        assert scan_wide_plan(dim, 8, nq, kp=8, sketch_wide=1)["passes"] == scan_matrix_plan(dim, 8, nq, kp=8)["passes"]
        assert scan_wide_plan(dim, 8, nq, kp=17)["passes"] == -(-nq // 16)


def test_rows_without_whole_steps_and_other_widths():
    for dim in (48, 100):
        assert not scan_wide_plan(dim, 8, 32, sketch_matrix=2, sketch_wide=2)["serves"], dim
    for bits in (4, 16, 32):
        assert not scan_wide_plan(768, bits, 32, sketch_matrix=2, sketch_wide=2)["serves"], bits


def test_option_range():
    for v in (0, 1, 2):
        option_check("sketch_wide", v)
    for v in (-1, 3, 4):
        with pytest.raises(SzgError):
            option_check("sketch_wide", v)
        with pytest.raises(SzgError):
            scan_wide_plan(768, 8, 32, sketch_wide=v)


@pytest.mark.parametrize("dim", DIMS)
def test_the_matrix_hook_answers_as_before(dim):
    for nq in (3, 16, 17, 32, 33, 40, 48, 96):
        for kp in (1, 8, 16, 17, 64):
            m = scan_matrix_plan(dim, 8, nq, kp=kp)
            assert m["serves"] and m["passes"] == -(-nq // 16), (dim, nq, kp, m)
            assert m["lds_bytes"] == lds_bytes(dim, kp, 1), (dim, nq, kp, m)
            assert m["steps"] == {64: 0, 384: 6, 768: 12}[dim], (dim, nq, kp, m)
