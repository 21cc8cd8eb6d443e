"""The matrix sketch sweep's selection, host only: which launches keep row lists (szg_debug_scan_select: scan_variant's
answer under option sketch_select) -- exactly those the matrix sweep serves with lists of at most 16 entries under
sketch_select = 0 -- and the option's range.  The option changes nothing the matrix hook reports: whether the sweep
serves, its passes, its STEPS form and its LDS bytes have no argument for it."""
import pytest

from syzgydb_amd import SzgError
from syzgydb_amd.index import scan_matrix_plan, scan_select_plan, option_check

DIMS = (64, 384, 768)
KPS = (1, 8, 16, 17, 64)
QUERIES = (3, 16, 40)
# launches the matrix sweep does not serve (test_sketch_matrix_cpu.py's)
NOT_SERVED = (("three planes", dict(planes=3)), ("no norms", dict(norms=False)), ("untiled", dict(tiled=False)),
              ("masked", dict(masked=True)), ("kp > 64", dict(kp=65)), ("kp = 96", dict(kp=96)),
              ("scan_group = 1", dict(scan_group=1)), ("scan_group = 2", dict(scan_group=2)),
              ("scan_group = 4", dict(scan_group=4)), ("sketch_matrix = 1", dict(sketch_matrix=1)))


@pytest.mark.parametrize("dim", DIMS)
def test_row_lists_where_served_and_short(dim):
    for nq in QUERIES:
        for kp in KPS:
            m = scan_matrix_plan(dim, 8, nq, kp=kp)
            assert m["serves"], (dim, nq, kp, m)
            for sel in (0, 1):
                p = scan_select_plan(dim, 8, nq, kp=kp, sketch_select=sel)
                what = (dim, nq, kp, sel, p)
                assert p["serves"] == m["serves"], what
                assert p["row_lists"] == (sel == 0 and kp <= 16), what
            # 16 two-plane images, their constants, 16 x waves lists of kp entries: no byte for the row lists
            assert m["lds_bytes"] == 16 * (2 * dim + 12 + 4 * kp * 8), (dim, nq, kp, m)
    for nq in (1, 2):   # sketch_matrix = 2 serves a lone query: row lists there too
        assert scan_select_plan(dim, 8, nq, sketch_matrix=2) == {"serves": True, "row_lists": True}
        assert scan_select_plan(dim, 8, nq, sketch_matrix=2, sketch_select=1) == {"serves": True, "row_lists": False}


@pytest.mark.parametrize("dim", DIMS)
def test_no_row_lists_where_not_served(dim):
    for sel in (0, 1):
        for nq in (1, 2):   # a lone query keeps the G = 1 kernel, two take G = 2
            assert scan_select_plan(dim, 8, nq, sketch_select=sel) == {"serves": False, "row_lists": False}, (dim, nq, sel)
        for nq in QUERIES:
            for why, kw in NOT_SERVED:
                kw = dict(dict(kp=8), **kw)
                p = scan_select_plan(dim, 8, nq, sketch_select=sel, **kw)
                assert p == {"serves": False, "row_lists": False}, (dim, nq, why, sel, p)
                assert not scan_matrix_plan(dim, 8, nq, **kw)["serves"], (dim, nq, why)


def test_rows_without_whole_steps_and_other_widths():
    for dim in (48, 100):
        for sm in (0, 2):
            assert not scan_select_plan(dim, 8, 16, sketch_matrix=sm)["row_lists"], (dim, sm)
    for bits in (4, 16, 32):
        assert scan_select_plan(768, bits, 16, sketch_matrix=2) == {"serves": False, "row_lists": False}, bits


def test_option_range():
    for v in (0, 1):
        option_check("sketch_select", v)
    for v in (-1, 2, 3):
        with pytest.raises(SzgError):
            option_check("sketch_select", v)
        with pytest.raises(SzgError):
            scan_select_plan(768, 8, 16, sketch_select=v)
    with pytest.raises(SzgError):   # (as the matrix hook refuses its option)
        scan_select_plan(768, 8, 16, sketch_matrix=3)
