"""Options "sketch_planes" and "scan_norms", checked on the host alone: the value ranges szg_set_option enforces
(szg_debug_option_check shares its check), and the plans of plain handles -- szg_debug_scan_group and szg_debug_scan_plan
describe a plain 8-bit handle, whose queries keep three digit planes.  (The two hooks take no handle and so no option:
what can be pinned here is that their answers are still the three-plane ones.)"""
import pytest

import scan_lattice as lat
from syzgydb_amd import option_check, scan_group_plan, scan_plan

KP = lat.kp_of(10)


def test_sketch_planes_range():
    for v in (0, 2, 3):
        option_check("sketch_planes", v)
    for v in (1, 4, -1):
        with pytest.raises(Exception):
            option_check("sketch_planes", v)


def test_scan_norms_range():
    for v in (0, 1):
        option_check("scan_norms", v)
    for v in (-1, 2):
        with pytest.raises(Exception):
            option_check("scan_norms", v)


def test_other_names_are_refused():
    option_check("scan_group", 4)
    with pytest.raises(Exception):
        option_check("scan_group", 3)
    with pytest.raises(Exception):
        option_check("no_such_option", 0)


def plans():
    out = {}
    for c in lat.cells(8):
        out[c.dim, "plan"] = scan_plan(c.dim, 8, c.small_n, KP)
        for nq in (1, 2, 3, 16, 17):
            for g in (0, 1, 2, 4):
                out[c.dim, nq, g] = scan_group_plan(c.dim, 8, nq, KP, scan_group=g)
    return out


def test_plain_handles_keep_their_plans():
    """The hooks answer for plain handles: a group's LDS is still three digit planes of r16 * 16 bytes per query
    beside the lists, and groups form as before (1, 2 or 4, never more than the launch can fill)."""
    base = plans()
    assert plans() == base   # (a pure function of its arguments)
    for c in lat.cells(8):
        p = base[c.dim, "plan"]
        waves = p["block"] // 64
        for nq in (2, 16):
            g = base[c.dim, nq, 0]
            assert g["group"] in (1, 2, 4) and g["group"] <= nq
            per_query = p["r16"] * 16 * 3 + waves * KP * 8
            assert g["lds_bytes"] == g["group"] * per_query + waves * 256 * 4, (c.dim, nq, g)
