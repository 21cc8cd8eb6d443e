"""The matrix sketch sweep's long-row form, host only (szg_debug_scan_long: scan_long_plan and scan_variant's answers for
ONE launch over 8-bit sketch rows).  Documented LDS (include/syzgy_scan.h): with b column blocks of 16 queries,
16 b (2 dim + 12 + 8 waves kp) bytes.  A form that fits 80 KiB runs blocks of 256 threads (4 waves), two to a CU; else one
block of 512 (8 waves) per CU within 160 KiB on half the grid; else it does not serve."""
import pytest

from syzgydb_amd.index import scan_long_plan, scan_matrix_plan, scan_wide_plan, scan_share_plan, scan_collect_plan

KIB = 1024


def lds_bytes(dim, kp, blocks, waves):
    return 16 * blocks * (2 * dim + 12 + 8 * waves * kp)


def planned(dim, kp, blocks):   # (threads, LDS bytes) of the form, None where it does not fit
    if lds_bytes(dim, kp, blocks, 4) <= 80 * KIB:
        return 256, lds_bytes(dim, kp, blocks, 4)
    if lds_bytes(dim, kp, blocks, 8) <= 160 * KIB:
        return 512, lds_bytes(dim, kp, blocks, 8)
    return None


def test_the_table_of_the_design():
    table = {1024: ((256, 37056), (256, 74112)), 1536: ((256, 53440), (512, 115072)), 2048: ((256, 69824), (512, 147840)),
             3072: ((512, 106688), None), 4096: ((512, 139456), None)}
    for dim, (one, two) in table.items():
        assert planned(dim, 8, 1) == one and planned(dim, 8, 2) == two, dim
        p = scan_long_plan(dim, 8, 32, kp=8)
        if dim < 1920:   # the one-block form of 64 KiB serves the shape: every launch keeps it (measured faster)
            assert not p["serves"] and p["passes"] == 2 and not scan_long_plan(dim, 8, 64, kp=8)["serves"], (dim, p)
            continue
        assert p["serves"] and p["blocks"] == (2 if two else 1) and p["passes"] == (1 if two else 2), (dim, p)
        assert (p["block"], p["lds_bytes"]) == (two or one), (dim, p)
        assert p["grid"] == (512 if p["block"] == 256 else 256), (dim, p)   # the hooks' 4M rows on 256 CUs
        s = scan_long_plan(dim, 8, 64, kp=8)
        assert s["share"] == bool(two) and s["passes"] == (2 if two else 4) and s["block"] == p["block"], (dim, s)


def test_short_rows_answer_as_before():
    for dim in (64, 384, 768, 960):
        for nq in (3, 16, 32, 64):
            assert not scan_long_plan(dim, 8, nq, kp=8)["serves"], (dim, nq)
    # 768 dimensions with lists of 16: two blocks are 384 bytes over 64 KiB and stay out
    w = scan_wide_plan(768, 8, 32, kp=16)
    assert not w["serves"] and w["passes"] == 2 and w["lds_bytes"] == lds_bytes(768, 16, 1, 4)
    assert lds_bytes(768, 16, 2, 4) == 64 * KIB + 384 and not scan_share_plan(768, 8, 64, kp=16, sketch_share=2)["serves"]
    for dim, kp in ((1024, 8), (1536, 16), (1856, 8)):
        m = scan_matrix_plan(dim, 8, 16, kp=kp)
        assert m["serves"] and m["lds_bytes"] == lds_bytes(dim, kp, 1, 4) <= 64 * KIB and m["steps"] == 0, (dim, m)
        assert not scan_long_plan(dim, 8, 16, kp=kp)["serves"], dim


@pytest.mark.parametrize("kp", (8, 16, 24))
def test_chosen_exactly_where_it_fits(kp):
    for dim in range(1024, 4096 + 64, 64):
        old = lds_bytes(dim, kp, 1, 4) <= 64 * KIB   # the one-block form of 64 KiB serves the shape: no long form
        one, two = planned(dim, kp, 1), planned(dim, kp, 2) if kp <= 16 and not old else None   # (row lists: 16 entries at most)
        p16, p32, p64 = (scan_long_plan(dim, 8, nq, kp=kp) for nq in (16, 32, 64))
        assert p16["serves"] == (not old and one is not None), (dim, kp, p16)
        if p16["serves"]:
            assert (p16["blocks"], p16["block"], p16["lds_bytes"], p16["passes"]) == (1,) + one + (1,), (dim, kp, p16)
        assert p32["blocks"] == p64["blocks"] == (2 if two else (1 if p16["serves"] else 0)), (dim, kp, p32, p64)
        if two:
            assert (p32["block"], p32["lds_bytes"], p32["passes"], p64["passes"]) == two + (1, 2), (dim, kp, p32, p64)
            assert p64["share"] and not p32["share"], (dim, kp)
    for dim in (4160, 8192):   # 65 steps and more: no matrix form
        assert not scan_long_plan(dim, 8, 16, kp=kp)["serves"] and not scan_matrix_plan(dim, 8, 16, kp=kp)["serves"], dim


def test_never_for_other_launches():
    for dim in (1024, 2048, 4096):
        for nq in (16, 32, 64):
            for why, kw in (("masked", dict(masked=True)), ("three planes", dict(planes=3)), ("no norms", dict(norms=False)),
                            ("untiled", dict(tiled=False))):
                assert not scan_long_plan(dim, 8, nq, **kw)["serves"], (dim, nq, why)
        assert not scan_long_plan(dim, 8, 2)["serves"] and scan_long_plan(dim, 8, 3)["serves"] == (dim > 1024)
        for bits in (4, 16, 32):
            assert not scan_long_plan(dim, bits, 32)["serves"], (dim, bits)
        c = scan_collect_plan(dim, 8, 32, sketch_wide=2)   # collect launches: the forms of 64 KiB or none
        assert not c["wide"] and c["serves"] == (dim == 1024) and c["lds_bytes"] <= 64 * KIB, (dim, c)
        assert scan_matrix_plan(dim, 8, 16, sketch_matrix=1)["serves"] is False


def test_a_rest_of_one_query_does_not_send_the_batch_back():
    """21 queries are launches of 16, 1 and 4: at a block of 512 each is one long pass (the grouped kernels: 4 + 1 + 1);
    a call of one or two queries keeps the one-query and two-query kernels."""
    for dim in (2048, 3072, 4096):
        p = scan_share_plan(dim, 8, 21, kp=8)
        assert (p["batches"], p["launches"], p["passes"]) == ([21], 3, 3), (dim, p)
        assert [scan_share_plan(dim, 8, nq, kp=8)["passes"] for nq in (1, 2, 3, 18)] == [1, 1, 1, 2], dim
