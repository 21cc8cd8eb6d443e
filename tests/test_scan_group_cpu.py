"""Groups of queries per row read (option "scan_group"), checked on the host alone through szg_debug_scan_group: which
launches form groups, what a group costs in LDS and how many passes over the rows a call makes -- the number
szg_stats.scan_bytes counts."""
import pytest

import scan_lattice as lat
from syzgydb_amd import SzgError, scan_group_plan, scan_plan
from syzgydb_amd._lib import SZG_E_INVALID

KP = lat.kp_of(10)


def passes(n, qpl, g):
    """n queries in launches of qpl, each launch in groups of g -- no larger than the launch can fill."""
    total = 0
    for j in range(0, n, qpl):
        m = min(qpl, n - j)
        e = g
        while e > 1 and e // 2 >= m:
            e //= 2
        total += -(-m // e)
    return total


@pytest.mark.parametrize("qpl", [1, 3, 4, 5, 16])
def test_pass_count_of_a_call(qpl):
    for g in (1, 2, 4):
        for n in (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 96):
            p = scan_group_plan(767, 8, n, KP, scan_group=g, queries_per_launch=qpl)
            assert p["passes"] == passes(n, qpl, g), (n, qpl, g, p)
            assert p["group"] == min(g, {1: 1, 2: 2}.get(min(n, qpl), 4)), (n, qpl, g, p)
    # hand-checked: 17 queries in launches of 16 at 4 per row read = 4 passes + 1; at 2 = 8 + 1
    if qpl == 16:
        assert scan_group_plan(767, 8, 17, KP, scan_group=4)["passes"] == 5
        assert scan_group_plan(767, 8, 17, KP, scan_group=2)["passes"] == 9
        assert scan_group_plan(767, 8, 17, KP, scan_group=1)["passes"] == 17
        assert scan_group_plan(767, 8, 3, KP, scan_group=4)["passes"] == 1


def test_automatic_is_one_of_the_sizes():
    auto = scan_group_plan(767, 8, 16, KP, scan_group=0)
    assert auto["group"] in (1, 2, 4)
    assert auto == scan_group_plan(767, 8, 16, KP, scan_group=auto["group"])
    assert scan_group_plan(767, 8, 1, KP, scan_group=0)["group"] == 1     # a lone query is never grouped


def test_only_unmasked_8bit_topk_with_register_lists_forms_groups():
    for bits in lat.WIDTHS:
        dim = lat.cells(bits)[-1].dim
        for kw in (dict(), dict(masked=True), dict(collect=True), dict(kp=lat.kp_of(80))):
            p = scan_group_plan(dim, bits, 16, **{"kp": KP, **kw}, scan_group=4)
            want = 4 if bits == 8 and not kw else 1
            assert p["group"] == want and p["passes"] == 16 // want, (bits, kw, p)
    for c in lat.cells(8):      # every lane-map class and both row-shape kernels
        assert scan_group_plan(c.dim, 8, 16, KP, scan_group=4)["group"] == 4, c
        assert scan_group_plan(c.dim, 8, 16, 64, scan_group=4)["group"] == 4, c     # the longest register lists


def test_lds_grows_with_the_group():
    """Per query of a group: its image (3 digit planes of 16 bytes per piece) and one list per wave; the waves' step
    lists (masked sweeps) are there once."""
    for c in lat.cells(8):
        p = scan_plan(c.dim, 8, 1 << 22, KP)
        waves = p["block"] // 64
        per_query = c.r16 * 48 + waves * KP * 8
        steps = waves * 256 * 4
        for g in (1, 2, 4):
            assert scan_group_plan(c.dim, 8, 16, KP, scan_group=g)["lds_bytes"] == g * per_query + steps, (c, g)


def test_a_group_that_does_not_fit_lds_is_halved():
    top = lat.max_dim(8)                               # 48 KiB of prepared query: no room for a second image
    assert scan_group_plan(top, 8, 16, KP, scan_group=4)["group"] == 1
    assert scan_group_plan(top, 8, 16, KP, scan_group=4)["passes"] == 16
    half = top // 2 - 128                              # two images fit beside the lists, four do not
    p = scan_group_plan(half, 8, 16, KP, scan_group=4)
    assert p["group"] == 2 and p["lds_bytes"] <= 64 * 1024 and p["passes"] == 8, p


def test_errors():
    for bad in (dict(scan_group=3), dict(scan_group=8), dict(scan_group=-1), dict(queries_per_launch=0),
                dict(queries_per_launch=17)):
        with pytest.raises(SzgError) as e:
            scan_group_plan(767, 8, 4, **{"kp": KP, **bad})
        assert e.value.code == SZG_E_INVALID
    with pytest.raises(SzgError) as e:
        scan_group_plan(767, 8, 0, KP)
    assert e.value.code == SZG_E_INVALID
