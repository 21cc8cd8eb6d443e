"""The row lists' whole-tile merge (option sketch_bulk), host only: the option's range, and that it has no way into the
routing -- the matrix, selection and wide hooks (scan_variant's answers, LDS bytes, passes) take no argument for it and
answer the same before and after every value has been through the option check."""
import inspect

import pytest

from syzgydb_amd import SzgError
from syzgydb_amd.index import scan_matrix_plan, scan_select_plan, scan_wide_plan, option_check

DIMS = (64, 384, 768)
KPS = (1, 8, 15, 16, 17)
QUERIES = (3, 16, 17, 32, 40)
ACCEPTED = (0, 1, 2, 48, 1024)
REFUSED = (-1, 1025)


def plans():
    out = {}
    for dim in DIMS:
        for nq in QUERIES:
            for kp in KPS:
                out[dim, nq, kp] = (scan_matrix_plan(dim, 8, nq, kp=kp), scan_select_plan(dim, 8, nq, kp=kp),
                                    scan_wide_plan(dim, 8, nq, kp=kp), scan_wide_plan(dim, 8, nq, kp=kp, sketch_wide=2))
    return out


def test_option_range():
    for v in ACCEPTED:
        option_check("sketch_bulk", v)
    for v in REFUSED:
        with pytest.raises(SzgError):
            option_check("sketch_bulk", v)


def test_plans_do_not_know_the_option():
    for hook in (scan_matrix_plan, scan_select_plan, scan_wide_plan):
        assert "sketch_bulk" not in inspect.signature(hook).parameters, hook.__name__
    before = plans()
    for v in ACCEPTED:
        option_check("sketch_bulk", v)
        assert plans() == before, v
    # (what the kernels under the option are: row lists up to 16 entries, the two-block form where it fits)
    assert before[768, 32, 8][1] == {"serves": True, "row_lists": True} and before[768, 32, 8][3]["serves"]
    assert before[768, 32, 17][1] == {"serves": True, "row_lists": False}
