"""A few 64-query sketch calls on the headline's handle (1M x 768 float32 cosine, k = 10) as ONE shared launch
(sketch_share = 2) or as two wide launches of 32 (sketch_share = 1), for a counter run (scripts/pmc.sh): per launch of
scan_mx_kernel the shared form's FETCH_SIZE, TCC hits and misses and instruction counts against the wide form's.
usage: python scripts/dev_share.py <sketch_share: 1 or 2> [queries] [rows] [dim]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle as orc  # noqa: E402
from syzgydb_amd import ScanIndex, SZG_COSINE  # noqa: E402

share = int(sys.argv[1]) if len(sys.argv) > 1 else 2
nq = int(sys.argv[2]) if len(sys.argv) > 2 else 64
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
dim = int(sys.argv[4]) if len(sys.argv) > 4 else 768
Q = orc.synth_vectors(11, 0, nq, dim)
with ScanIndex(dim, 32, SZG_COSINE) as ix:
    ix.synth(n, 7)
    for name, v in (("multi_query", 0), ("sketch", 1), ("sketch_matrix", 2), ("sketch_wide", 2), ("sketch_share", share)):
        ix.set_option(name, v)
    ix.search_topk(Q[:16], 10)   # builds the sketch and the norms
    ix.reset_stats()
    for _ in range(8):
        ix.search_topk(Q, 10)
    st = ix.stats()
    print("sketch_share %d  queries %d  launches/call %.1f  passes/call %.1f  settled %d/%d" % (
        share, nq, st["scan_launches"] / 8, st["scan_bytes"] / (n * dim) / 8, st["sketch_queries"], 8 * nq))
