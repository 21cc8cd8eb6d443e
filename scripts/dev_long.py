"""Sweep time of top-k calls through the sketch of a float32 collection of long rows (1 024 .. 4 096 dimensions), for the
library selected by SZG_LIB_PATH (A/B of builds: run once per library, alternating, inside ONE GPU call).
  python scripts/dev_long.py rows:dim[:metric] ...      SZG_OPTS=name=v,... applies options; SZG_NQS=1024,16 the calls
Per shape and call size: HIP-event time of the call's sweeps (szg_stats.scan_ms, best and median of SZG_REPS calls), the
passes over the sketch rows, the time per pass and launch, and the wall time of the call."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from syzgydb_amd import ScanIndex
tag = os.path.basename(os.environ.get("SZG_LIB_PATH", "tree")).replace("libsyzgy_scan_", "").replace(".so", "")
nqs = [int(x) for x in os.environ.get("SZG_NQS", "1024,16").split(",")]
reps = int(os.environ.get("SZG_REPS", "7"))
for spec in sys.argv[1:]:
    f = [int(x) for x in spec.split(":")]
    n, dim, metric = f[0], f[1], (f[2] if len(f) > 2 else 1)
    Q = np.random.default_rng(99).uniform(-1, 1, (max(nqs), dim))
    with ScanIndex(dim, 32, metric, devices=[0]) as ix:
        # (the sketch is built as the rows arrive: its options come first; multi_query = 0 keeps long calls on the one-sweep path)
        for name, val in [("sketch", 1), ("sketch_min_rows", 1), ("multi_query", 0)] + [x.split("=") for x in os.environ.get("SZG_OPTS", "").split(",") if x]:
            ix.set_option(name, int(val))
        ix.synth(n, 1234)
        for nq in nqs:
            q = Q[:nq]
            ix.search_topk(q, 10); ix.search_topk(q, 10)
            ms, wall = [], []
            for rep in range(reps):
                ix.set_timing(True); ix.reset_stats()
                t0 = time.perf_counter(); ix.search_topk(q, 10); wall.append(1e3 * (time.perf_counter() - t0))
                s = ix.stats(); ix.set_timing(False)
                ms.append(s["scan_ms"])
            passes = s["scan_bytes"] / float(n * dim)
            print("%-8s %8d x %4d m%d nq %4d: sweeps %8.3f ms best %8.3f median  %5.1f passes %3d launches  %7.1f us/pass  wall %8.2f ms best"
                  "  settled %d fallbacks %d" % (tag, n, dim, metric, nq, min(ms), sorted(ms)[len(ms) // 2], passes, s["scan_launches"],
                                              1e3 * min(ms) / max(passes, 1), min(wall), s["sketch_queries"], s["sketch_fallbacks"]), flush=True)
