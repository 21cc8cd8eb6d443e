#!/usr/bin/env python3
"""Every decision of the one-sweep scan's plan over a grid, one line per point, host only (no device is opened): the
answers of scan_plan, scan_group_plan, scan_matrix_plan, scan_select_plan, scan_wide_plan, scan_collect_plan,
scan_group_ring_plan and merge_short_plan.  Two builds of the library decide alike where their outputs are equal byte
for byte:

    SZG_LIB_PATH=old/libsyzgy_scan.so scripts/scan_plan_table.py | sha256sum
    scripts/scan_plan_table.py | sha256sum

--lines prints the table itself (several million lines); the default is its line count and SHA-256.
The library's tuning constants `ring` and `shape_kernels` are compile-time constants of the handle (scan_internal.h), no
option of szg_set_option names them: the table covers the values the library is built with; ring >= 8 and
no_shape_kernels are exercised by tests/cpp/test_scan_plan.cpp."""
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from syzgydb_amd import SzgError, scan_lattice  # noqa: E402
from syzgydb_amd.index import (merge_short_plan, scan_collect_plan, scan_group_plan, scan_group_ring_plan,  # noqa: E402
                               scan_matrix_plan, scan_plan, scan_select_plan, scan_wide_plan)

WIDTHS = (4, 8, 16, 32, 64)
DIMS = (1, 63, 64, 128, 192, 384, 768, 1024, 1536)
KPS = (0, 1, 8, 15, 16, 17, 64, 65, 128)
NQS = (1, 2, 3, 4, 16, 17, 32, 33, 64)
ON_OFF = (False, True)
GROUPS = (0, 1, 2, 4)
MATRIX = (0, 1, 2)
SELECT = (0, 1)
WIDE = (0, 1, 2)


def answer(fn, *args, **kw):
    try:
        r = fn(*args, **kw)
    except SzgError as e:
        return "error %d" % e.code
    return " ".join("%s=%s" % (k, int(v) if isinstance(v, bool) else v) for k, v in r.items())


def table():
    for bits in WIDTHS:
        dims = DIMS + (scan_lattice.max_dim(bits),)
        rings = [0] + scan_group_ring_plan(768, bits, 1)["depths"]
        for dim in dims:
            head = "%d %d" % (bits, dim)
            for kp, collect, masked in itertools.product(KPS, ON_OFF, ON_OFF):
                yield "plan %s kp=%d c=%d m=%d: %s" % (head, kp, collect, masked,
                                                     answer(scan_plan, dim, bits, 1 << 22, kp, collect, masked))
                for nq, group in itertools.product(NQS, GROUPS):
                    yield "group %s kp=%d c=%d m=%d nq=%d g=%d: %s" % (
                        head, kp, collect, masked, nq, group,
                        answer(scan_group_plan, dim, bits, nq, kp, group, 16, collect, masked))
            for kp, nq, group, ring in itertools.product(KPS, NQS, GROUPS, rings):
                if nq <= 16:
                    yield "ring %s kp=%d nq=%d g=%d r=%d: %s" % (head, kp, nq, group, ring,
                                                               answer(scan_group_ring_plan, dim, bits, nq, kp, group, ring))
            for nq, planes, norms, tiled, masked, group, matrix in itertools.product(NQS, (2, 3), ON_OFF, ON_OFF, ON_OFF,
                                                                                       GROUPS, MATRIX):
                shape = (planes, norms, tiled, masked, group, matrix)
                tail = "%s nq=%d p=%d n=%d t=%d m=%d g=%d mx=%d" % ((head, nq) + shape)
                for wide in WIDE:
                    yield "collect %s w=%d: %s" % (tail, wide, answer(scan_collect_plan, dim, bits, nq, *shape, wide))
                for kp in KPS:
                    yield "matrix %s kp=%d: %s" % (tail, kp, answer(scan_matrix_plan, dim, bits, nq, kp, *shape))
                    for select in SELECT:
                        yield "select %s kp=%d s=%d: %s" % (tail, kp, select,
                                                          answer(scan_select_plan, dim, bits, nq, kp, *shape, select))
                        for wide in WIDE:
                            yield "wide %s kp=%d s=%d w=%d: %s" % (
                                tail, kp, select, wide, answer(scan_wide_plan, dim, bits, nq, kp, *shape, select, wide))
    for n_lists, m, kp in itertools.product((0, 1, 63, 64, 65, 512, 1023, 1024, 1025), (0, 1, 7, 8, 15, 16, 63, 64),
                                            KPS + (256, 4096)):
        yield "merge_short %d %d %d: %s" % (n_lists, m, kp, answer(merge_short_plan, n_lists, m, kp))


def main():
    lines = "--lines" in sys.argv[1:]
    h, n = hashlib.sha256(), 0
    for line in table():
        if lines:
            print(line)
        h.update(line.encode() + b"\n")
        n += 1
    if not lines:
        print("%d lines, sha256 %s" % (n, h.hexdigest()))


if __name__ == "__main__":
    main()
