"""The matrix sketch sweep's routing, host only: which one-sweep launches scan_variant hands to the matrix kernel
(szg_debug_scan_matrix), their passes over the rows and LDS, and the range of option sketch_matrix."""
import pytest

from syzgydb_amd import SzgError
from syzgydb_amd.index import scan_matrix_plan, scan_group_plan, option_check

DIMS = {768: 12, 384: 6, 64: 0}   # dimension -> STEPS form (0: the any-steps kernel)
QUERIES = (3, 4, 15, 16, 17, 18, 19, 32, 40, 96)


@pytest.mark.parametrize("dim", sorted(DIMS))
def test_served(dim):
    for nq in QUERIES:
        for kp in (1, 8, 56, 64):
            p = scan_matrix_plan(dim, 8, nq, kp=kp)
            what = (dim, nq, kp, p)
            assert p["serves"] and p["steps"] == DIMS[dim], what
            assert p["passes"] == -(-nq // 16), what
            assert 0 < p["lds_bytes"] <= 64 * 1024, what
            # 16 two-plane images, their constants, 16 x waves lists of kp entries (4 waves per block)
            assert p["lds_bytes"] == 16 * (2 * dim + 12 + 4 * kp * 8), what
    # sketch_matrix = 2: wherever the shape allows, a lone query included
    for nq in (1, 2):
        assert scan_matrix_plan(dim, 8, nq, sketch_matrix=2)["serves"]


@pytest.mark.parametrize("dim", sorted(DIMS))
def test_not_served(dim):
    for nq in (1, 2):   # a lone query keeps the G = 1 kernel, two take G = 2
        p = scan_matrix_plan(dim, 8, nq)
        assert not p["serves"] and p["passes"] == 1, (dim, nq, p)
    for nq in (3, 16, 40):
        grouped = scan_group_plan(dim, 8, nq, kp=8)["passes"]
        for why, kw in (("three planes", dict(planes=3)), ("no norms", dict(norms=False)), ("untiled", dict(tiled=False)),
                        ("masked", dict(masked=True)), ("kp > 64", dict(kp=65)), ("kp = 96", dict(kp=96)),
                        ("scan_group = 1", dict(scan_group=1)), ("scan_group = 2", dict(scan_group=2)),
                        ("scan_group = 4", dict(scan_group=4)), ("sketch_matrix = 1", dict(sketch_matrix=1))):
            p = scan_matrix_plan(dim, 8, nq, **dict(dict(kp=8), **kw))
            assert not p["serves"] and p["steps"] == 0, (dim, nq, why, p)
            if why in ("three planes", "no norms", "sketch_matrix = 1", "scan_group = 4"):
                assert p["passes"] == grouped, (dim, nq, why, p, grouped)   # the grouped kernels, as before
            if why == "masked":
                assert p["passes"] == nq, (dim, nq, why, p)


@pytest.mark.parametrize("dim", (48, 100))
def test_rows_without_whole_steps(dim):
    for nq in (3, 16):
        for sm in (0, 2):
            p = scan_matrix_plan(dim, 8, nq, sketch_matrix=sm)
            assert not p["serves"], (dim, nq, sm, p)


def test_other_row_widths():
    for bits in (4, 16, 32):
        assert not scan_matrix_plan(768, bits, 16, sketch_matrix=2)["serves"]


def test_group_hook_unchanged():
    """szg_debug_scan_group does not know the matrix sweep: its answers are the grouped kernels'."""
    assert scan_group_plan(768, 8, 16, kp=8) == {"group": 4, "lds_bytes": scan_group_plan(768, 8, 16, kp=8)["lds_bytes"], "passes": 4}
    assert scan_group_plan(768, 8, 3, kp=8)["group"] == 4 and scan_group_plan(768, 8, 1, kp=8)["group"] == 1


def test_option_range():
    for v in (0, 1, 2):
        option_check("sketch_matrix", v)
    for v in (-1, 3):
        with pytest.raises(SzgError):
            option_check("sketch_matrix", v)
        with pytest.raises(SzgError):
            scan_matrix_plan(768, 8, 16, sketch_matrix=v)
