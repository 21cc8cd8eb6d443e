"""The scan kernel's shape lattice, checked on the host alone (szg_debug_scan_plan needs no device): every lane-map
class the heuristic can produce has a cell in tests/scan_lattice.py, the row counts chosen for the cells reach the
phases they are meant to reach, and the assumptions the kernel's tests rest on (power-of-two lane groups only) still
hold.  A change to choose_map, scan_geometry or the launcher's variant choice that opens a new path fails here first."""
import pytest

import scan_lattice as lat
from syzgydb_amd import SzgError, scan_plan
from syzgydb_amd._lib import SZG_E_INVALID, SZG_E_UNSUPPORTED

# what a transcription of choose_map and the row-size rules predicts (4- and 8-bit rows of whole 64-byte steps are
# tiled, which folds L = 8 / 16 / 32 / 64 dense maps into the tiled L = 4 ones)
EXPECTED_CLASSES = {4: 15, 8: 15, 16: 17, 32: 17, 64: 17}
EXPECTED_SHAPES = {4: [403, 406], 8: [406, 412], 16: [], 32: [812], 64: []}


@pytest.mark.parametrize("bits", lat.WIDTHS)
def test_every_class_has_a_cell(bits):
    have = {c.cls for c in lat.cells(bits) if c.kind == "class"}
    for p in lat.walk(bits):
        assert lat.class_of(p) in have, "lane-map class %r (r16 = %d) has no lattice cell" % (lat.class_of(p), p["r16"])
    assert len(have) == EXPECTED_CLASSES[bits], sorted(have)
    ragged = [c for c in have if c[3] == "ragged"]
    assert len(ragged) == 9, ragged
    for c in lat.cells(bits):
        assert c.dim % 2 == 1 or (bits == 64 and c.r16 == 1)
        assert scan_plan(c.dim, bits, c.small_n)["r16"] == c.r16
        assert scan_plan(c.dim + 1, bits, c.small_n)["r16"] in (c.r16, c.r16 + 1)


@pytest.mark.parametrize("bits", lat.WIDTHS)
def test_only_power_of_two_lane_groups(bits):
    for p in lat.walk(bits):
        assert p["pow2"] == 1 and p["L"] in (1, 2, 4, 8, 16, 32, 64) and p["L"] * p["gpw"] == 64, (
            "r16 = %d of %d-bit rows maps to L = %d, pow2 = %d: a new kind of lane map (grp_sum's shuffle reduction, "
            "groups that do not fill the wave) that no test has run -- it needs lattice cells of its own" %
            (p["r16"], bits, p["L"], p["pow2"]))
        assert p["L"] * p["P"] >= p["r16"] and p["L"] * (p["P"] - 1) < p["r16"], p
        assert p["dense"] == (1 if p["L"] * p["P"] == p["r16"] else 0), p
        if p["tiled"]:
            assert bits <= 8 and p["r16"] % 4 == 0 and p["L"] == 4 and p["dense"] == 1, p
        assert p["nontemporal"] == (1 if p["L"] >= 8 or p["tiled"] else 0), p


@pytest.mark.parametrize("bits", lat.WIDTHS)
def test_deep_rows_reach_the_dense_phase(bits):
    """From the plan's own numbers: at a cell's deep n every wave has steps * P >= 2 * D pieces of whole row steps --
    the dense phase's entry condition -- in the unmasked, the masked and the collect sweep, and n leaves a partial
    group and a partial mask word."""
    for c in lat.cells(bits):
        n = c.deep_n
        for kw in (dict(), dict(masked=True), dict(collect=True), dict(collect=True, masked=True)):
            p = scan_plan(c.dim, bits, n, lat.kp_of(lat.DEEP_K), **kw)
            steps = n // (p["grid"] * p["rows_per_block"])   # whole steps of the wave that starts last
            assert steps * p["P"] >= 2 * p["ring_depth"], (c, kw, p)
            assert steps >= 2, (c, kw, p)                       # several rows per wave
            assert p["ring_depth"] in (3, 4, 6), p
        p = scan_plan(c.dim, bits, n, lat.kp_of(lat.DEEP_K))
        assert n // (p["grid"] * p["rows_per_block"]) == c.deep_steps == -(-2 * p["ring_depth"] // p["P"]) + 2
        assert n % 64 != 0 and (c.gpw == 1 or n % c.gpw != 0), c
        # (a deep cell stays a few tens of MiB)
        assert n * (c.r16 * 16) < 128 << 20, "deep cell of %d MiB" % (n * c.r16 * 16 >> 20)


@pytest.mark.parametrize("bits", lat.WIDTHS)
def test_small_rows_take_one_step_per_wave(bits):
    for c in lat.cells(bits):
        p = scan_plan(c.dim, bits, c.small_n, lat.kp_of(10))
        assert p["block"] == 256 and p["rows_per_block"] == 4 * c.gpw
        assert c.small_n == 3 * p["rows_per_block"] + (c.gpw + 1) // 2
        assert p["grid"] == 4                                # three full blocks and a partial group in the fourth
        assert c.small_n % p["rows_per_block"] != 0


@pytest.mark.parametrize("bits", lat.WIDTHS)
def test_deep_ring_cells(bits):
    """k = 80 keeps more than 64 candidates per list: every cell then runs the any-shape kernel with the deep ring."""
    assert lat.kp_of(80) > 64 >= lat.kp_of(10)
    for c in lat.cells(bits):
        for masked in (False, True):
            p = scan_plan(c.dim, bits, c.small_n, lat.kp_of(80), masked=masked)
            assert p["ring_depth"] == 8 and p["shaped"] == 0, (c, p)
        # a collect sweep keeps no lists: the short ring whatever k was
        assert scan_plan(c.dim, bits, c.small_n, lat.kp_of(80), collect=True)["ring_depth"] in (3, 4, 6)


@pytest.mark.parametrize("bits", lat.WIDTHS)
def test_specialised_shapes(bits):
    assert sorted(lat.shapes(bits)) == EXPECTED_SHAPES[bits]
    shape_cells = {c.shaped: c for c in lat.cells(bits) if c.kind == "shape"}
    assert sorted(shape_cells) == EXPECTED_SHAPES[bits]
    for code, c in shape_cells.items():
        assert code == c.L * 100 + c.P and c.dense
        for n in (c.small_n, c.deep_n):
            assert scan_plan(c.dim, bits, n, lat.kp_of(10))["shaped"] == code
            assert scan_plan(c.dim, bits, n, lat.kp_of(10), collect=True)["shaped"] == code
            assert scan_plan(c.dim, bits, n, lat.kp_of(10), masked=True)["shaped"] == 0
            assert scan_plan(c.dim, bits, n, lat.kp_of(10), collect=True, masked=True)["shaped"] == 0
        assert c.P % scan_plan(c.dim, bits, c.deep_n, lat.kp_of(10))["ring_depth"] == 0   # the row-unrolled ring


def test_limits_and_errors():
    for bits in lat.WIDTHS:
        top = lat.max_dim(bits)
        assert scan_plan(top, bits, 100)["r16"] == len(lat.walk(bits))
        with pytest.raises(SzgError) as e:
            scan_plan(top + 1, bits, 100)
        assert e.value.code == SZG_E_UNSUPPORTED
    assert [lat.max_dim(b) for b in lat.WIDTHS] == [24576, 16384, 12288, 12288, 6144]   # 48 KiB of prepared query
    for bad in (dict(dim=0, quant_bits=32), dict(dim=8, quant_bits=5), dict(dim=(1 << 20) + 1, quant_bits=4)):
        with pytest.raises(SzgError) as e:
            scan_plan(n_rows=10, **bad)
        assert e.value.code == SZG_E_INVALID


def test_grid_follows_rows_and_card():
    p = scan_plan(128, 32, 5000, lat.kp_of(10))
    assert (p["L"], p["P"], p["gpw"], p["block"]) == (8, 4, 8, 256)
    assert p["grid"] == -(-5000 // p["rows_per_block"])       # below the cap: one step per wave, no dense phase (P = 4)
    big = scan_plan(128, 32, 1 << 30, lat.kp_of(10))
    assert big["grid"] == 256 * 3                             # 12 waves per CU on the default 256
    assert scan_plan(128, 32, 1 << 30, lat.kp_of(10), cu_count=64)["grid"] == 64 * 3
    assert scan_plan(768, 32, 1 << 30, lat.kp_of(10))["grid"] == 256 * 2     # float rows of >= 1 KiB: 8 waves per CU
    assert scan_plan(128, 32, 1 << 30, lat.kp_of(80))["grid"] == 256 * 2     # lists in LDS: 8 waves per CU
    assert scan_plan(1, 32, 0, 1)["grid"] == 1
