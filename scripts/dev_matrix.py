"""Launch times of the sketch sweep by the library's HIP events, matrix sweep against the grouped kernels:
1M x 768 float32 cosine (the headline's handle), calls of 1, 2, 3, 4, 16 and 32 queries under sketch_matrix = 2 (the
matrix sweep whatever the count) with row lists (sketch_select = 0) and with the serial inserts (sketch_select = 1),
and under sketch_matrix = 1 (G = 1, 2, 4) -- all three with sketch_wide = 1 -- and the wide column: the two-block form
(sketch_wide = 2, row lists) at 17, 32, 48 and 64 queries, one launch per 32.  The share column: the shared form
(sketch_wide = 2, sketch_share = 2) at 33, 48 and 64 queries in ONE launch, beside the wide column's 64 (two launches).  SZG_NO_EARLY_TAIL=1 keeps a 16-query
call one launch.  The rows and wide columns run under sketch_bulk = 1 (rounds only) and 0 (crowded tiles merged whole), and
with SZG_BULK_SWEEP=1 under the thresholds 32, 48, 64, 96 and 128 as well.  A library from before sketch_select, sketch_wide
or sketch_bulk (an A/B run through SZG_LIB_PATH) shows what it has.
usage: SZG_NO_EARLY_TAIL=1 [SZG_BULK_SWEEP=1] python scripts/dev_matrix.py [rows] [dim]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle as orc  # noqa: E402
from syzgydb_amd import ScanIndex, SZG_COSINE  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
Q = orc.synth_vectors(11, 0, 64, dim)
BULK_SWEEP = (32, 48, 64, 96, 128)
with ScanIndex(dim, 32, SZG_COSINE) as ix:
    ix.synth(n, 7)
    for name, v in (("multi_query", 0), ("sketch", 1)):
        ix.set_option(name, v)
    ix.search_topk(Q[:16], 10)   # builds the sketch and the norms
    ix.set_timing(1)
    def measure(label, counts):
        for nq in counts:
            for _ in range(3):
                ix.search_topk(Q[:nq], 10)
            ix.reset_stats()
            reps = 20
            for _ in range(reps):
                ix.search_topk(Q[:nq], 10)
            st = ix.stats()
            passes = st["scan_bytes"] / (n * dim)
            print("%-10s queries %2d  launches/call %.1f  passes/call %.1f  ms/launch %.4f  ms/pass %.4f  settled %d/%d" % (
                label, nq, st["scan_launches"] / reps, passes / reps, st["scan_ms"] / max(st["timed_launches"], 1),
                st["scan_ms"] / max(passes, 1), st["sketch_queries"], reps * nq), flush=True)

    for sm, sel, label in ((2, 0, "rows"), (2, 0, "wide"), (2, 0, "share"), (2, 1, "serial"), (1, 0, "grouped")):
        ix.set_option("sketch_matrix", sm)
        try:
            ix.set_option("sketch_wide", 2 if label in ("wide", "share") else 1)
        except Exception:
            if label in ("wide", "share"):
                continue
        # the shared form (option sketch_share = 2): 33, 48 and 64 queries in ONE launch of two column groups on paired
        # blocks, beside the wide column's "64" (two launches); every other column keeps it off
        try:
            ix.set_option("sketch_share", 2 if label == "share" else 1)
        except Exception:
            if label == "share":
                continue
        if label == "share":
            measure("share", (33, 48, 64))
            continue
        try:
            ix.set_option("sketch_select", sel)
        except Exception:
            if sel:
                continue
            label = "matrix"
        counts = (17, 32, 48, 64) if label == "wide" else (1, 2, 3, 4, 16, 32, 64)
        # the row lists' whole-tile merge (option sketch_bulk): rounds only (1), automatic (0) and the threshold sweep --
        # the one-block form at 1 .. 16 queries, the two-block form at 17 .. 64; a library from before it shows what it has
        bulks = (1, 0) + (BULK_SWEEP if os.environ.get("SZG_BULK_SWEEP") else ()) if label in ("rows", "wide") else (None,)
        for bulk in bulks:
            tag = label
            if bulk is not None:
                try:
                    ix.set_option("sketch_bulk", bulk)
                    tag = "%s b%d" % (label, bulk)
                except Exception:
                    if bulk != 1:
                        continue
            measure(tag, (1, 2, 3, 4, 16) if label == "rows" and bulk not in (None, 1) else counts)
        try:
            ix.set_option("sketch_bulk", 0)
        except Exception:
            pass
