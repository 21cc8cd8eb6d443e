"""The shape lattice of the one-sweep scan kernel (kernels_scan.hip), derived from the library's own launch rules.

scan_plan() -- the host-only hook szg_debug_scan_plan -- answers for any (dim, row width, rows, kp, collect, masked)
with the lane map choose_map picks, the grid scan_geometry picks and the kernel variant the launcher picks.  This
module walks every row size a width accepts, groups the lane maps into classes

    (tiled or linear, L lanes per row, P == 1 or P > 1 pieces per lane, dense L*P == r16 or ragged L*P > r16)

and keeps one cell per class -- the smallest r16 of the class -- plus one cell per row-shape-specialised kernel.  A cell's
dimension is the largest odd one that maps to its r16, so the row's last 16-byte piece is partly padding.  For each
cell two row counts follow from the plan:

    small  three wave steps of one block plus a partial group: every launch variant, one step per wave
    deep   the smallest n at which EVERY wave walks ceil(2*D/P) + 2 row steps (D = ring depth), so the predicate-free
           dense phase runs, over several rows per wave, and hands a remainder to the general phase

The tests reach it as tests/scan_lattice.py (which also prints the lattice), the fuzzer (scripts/fuzz_gpu.py) draws its
dimensions from it.  Test support, like synth.py: nothing on the search path imports it.
"""
import functools
from collections import namedtuple

from ._lib import SZG_E_UNSUPPORTED, SzgError
from .index import scan_plan

WIDTHS = (4, 8, 16, 32, 64)
KS = (1, 10, 80)           # k = 80 keeps kp = 120 > 64 candidates per list: they live in LDS and the ring is deep
DEEP_K = 10

Cell = namedtuple("Cell", "bits kind cls r16 dim L P gpw tiled dense shaped small_n deep_n deep_steps ring_depth")


def kp_of(k):
    """Candidates per list of a top-k sweep at the default slack (TopkCall::run: k + max(slack_min = 16, k / 2))."""
    return k + max(16, k // 2)


def elements_per_piece(bits):
    return 128 // bits


@functools.lru_cache(maxsize=None)
def walk(bits):
    """The plan of every r16 the width accepts (full pieces, kp of k = 10), up to the limit on the LDS-resident query."""
    plans = []
    r16 = 1
    while True:
        try:
            p = scan_plan(r16 * elements_per_piece(bits), bits, 1 << 22, kp_of(DEEP_K))
        except SzgError as e:
            if e.code != SZG_E_UNSUPPORTED:
                raise
            break
        assert p["r16"] == r16, (bits, r16, p)
        plans.append(p)
        r16 += 1
    return plans


def max_dim(bits):
    """The largest dimension szg_index_create accepts for the width."""
    return len(walk(bits)) * elements_per_piece(bits)


def class_of(p):
    ragged = p["L"] * p["P"] > p["r16"]
    return ("tiled" if p["tiled"] else "linear", p["L"], "P=1" if p["P"] == 1 else "P>1", "ragged" if ragged else "dense")


def cell_dim(bits, r16):
    """The largest odd dimension that maps to r16 (the last piece is partly padding); one whole piece for 64-bit rows
    of a single piece, where the odd dimension would be 1 and every cosine distance 0 or 1."""
    if bits == 64 and r16 == 1:
        return 2
    return r16 * elements_per_piece(bits) - 1


def small_rows(p):
    return 3 * p["rows_per_block"] + (p["gpw"] + 1) // 2


def deep_rows(dim, bits, extra_steps=2):
    """(n, steps): the smallest n at which every wave of the top-k sweep at k = 10 walks `steps` = ceil(2*D/P) +
    extra_steps full row steps, moved up to the next n with n % gpw != 0 (where gpw > 1) and n % 64 != 0."""
    p = scan_plan(dim, bits, 1 << 40, kp_of(DEEP_K))   # (so many rows that the grid is the cap of the card)
    steps = -(-2 * p["ring_depth"] // p["P"]) + extra_steps
    n = steps * p["grid"] * p["rows_per_block"]
    while n % 64 == 0 or (p["gpw"] > 1 and n % p["gpw"] == 0):
        n += 1
    return n, steps


def _cell(bits, kind, r16):
    dim = cell_dim(bits, r16)
    p = scan_plan(dim, bits, 1 << 22, kp_of(DEEP_K))
    assert p["r16"] == r16, (bits, dim, p)
    n, steps = deep_rows(dim, bits)
    return Cell(bits, kind, class_of(p), r16, dim, p["L"], p["P"], p["gpw"], p["tiled"], p["dense"], p["shaped"],
                small_rows(p), n, steps, p["ring_depth"])


@functools.lru_cache(maxsize=None)
def classes(bits):
    """class -> smallest r16 of the class, over every r16 the width accepts."""
    first = {}
    for p in walk(bits):
        first.setdefault(class_of(p), p["r16"])
    return first


@functools.lru_cache(maxsize=None)
def shapes(bits):
    """shaped code -> r16 of every row-shape-specialised kernel of the width."""
    first = {}
    for p in walk(bits):
        if p["shaped"]:
            first.setdefault(p["shaped"], p["r16"])
    return first


@functools.lru_cache(maxsize=None)
def cells(bits):
    out = [_cell(bits, "class", r16) for r16 in sorted(classes(bits).values())]
    seen = {c.r16 for c in out}
    for code, r16 in sorted(shapes(bits).items()):
        if r16 not in seen:
            out.append(_cell(bits, "shape", r16))
    return out


def all_cells():
    return [c for bits in WIDTHS for c in cells(bits)]


def cell_id(c):
    return "%db-r%d-%s%d%s%s%s" % (c.bits, c.r16, "T" if c.tiled else "L", c.L, "p1" if c.P == 1 else "pn",
                                   "d" if c.L * c.P == c.r16 else "r", "-shape%d" % c.shaped if c.kind == "shape" else "")


def edge_cells(bits):
    """One dense and one ragged cell of the width for the row-count edges: the shortest row among the cells with 16 or
    more rows per wave step (1, gpw - 1, gpw, gpw + 1 and rows_per_block -+ 1 are then six different counts)."""
    out = []
    for want in ("dense", "ragged"):
        cand = [c for c in cells(bits) if c.cls[3] == want and c.kind == "class"]
        out.append(max(cand, key=lambda c: (min(c.gpw, 16), -c.r16)))
    return out


def edge_rows(c):
    rpb = scan_plan(c.dim, c.bits, 1 << 22, kp_of(DEEP_K))["rows_per_block"]
    return sorted({n for n in (1, c.gpw - 1, c.gpw, c.gpw + 1, rpb - 1, rpb + 1) if n >= 1})


def main():
    for bits in WIDTHS:
        print("%d-bit rows: r16 1..%d, largest dim %d, %d classes, shape kernels %s"
              % (bits, len(walk(bits)), max_dim(bits), len(classes(bits)), sorted(shapes(bits))))
        print("  %-26s %5s %5s %3s %3s %3s %7s %8s %5s" % ("class / shape", "r16", "dim", "L", "P", "gpw", "small n", "deep n", "steps"))
        for c in cells(bits):
            name = "%s L=%d %s %s" % c.cls if c.kind == "class" else "shape %d" % c.shaped
            print("  %-26s %5d %5d %3d %3d %3d %7d %8d %5d" % (name, c.r16, c.dim, c.L, c.P, c.gpw, c.small_n, c.deep_n,
                                                                c.deep_steps))
