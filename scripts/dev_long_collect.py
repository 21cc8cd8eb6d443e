"""Sweep time of radius calls (sketch_radius = 1, radius_mq = 0) and of top-k calls of k = 100 (sketch_topk_collect = 1)
through the sketch of a float32 collection of long rows (2 048 .. 4 096 dimensions), for the library selected by
SZG_LIB_PATH (A/B of builds: run once per library, alternating, inside ONE GPU call -- scripts/dev_long.py's way).
  python scripts/dev_long_collect.py rows:dim[:metric] ...      SZG_OPTS=name=v,... applies options; SZG_NQ=1024 the call
The radii are each query's 25th float64 distance (a top-k call finds them): a few dozen hits per query.
Per shape and mode: HIP-event time of the call's sweeps (szg_stats.scan_ms; best, median and worst of the timed calls --
after one warm-up call, calls are timed until there are SZG_REPS of them AND their sweeps add up to SZG_MIN_MS, 200 at the
most), the bytes swept in sketch rows ("passes"), queries per second of sweep time, the wall time, what the sketch settled,
and a hash of the answer (every query's rows and float64 distances): two builds that print the same hash for a shape and
mode returned the same answer, bit for bit."""
import hashlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from syzgydb_amd import ScanIndex
tag = os.path.basename(os.environ.get("SZG_LIB_PATH", "tree")).replace("libsyzgy_scan_", "").replace(".so", "")
nq = int(os.environ.get("SZG_NQ", "1024"))
reps = int(os.environ.get("SZG_REPS", "20"))
min_ms = float(os.environ.get("SZG_MIN_MS", "1000"))
opts = [x.split("=") for x in os.environ.get("SZG_OPTS", "").split(",") if x]


def answer_hash(mode, got):
    h = hashlib.sha1()
    parts = [x for pair in got for x in pair] if mode == "radius" else [got[0], got[1], got[2]]
    for x in parts:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()[:12]


for spec in sys.argv[1:]:
    f = [int(x) for x in spec.split(":")]
    n, dim, metric = f[0], f[1], (f[2] if len(f) > 2 else 1)
    Q = np.random.default_rng(99).uniform(-1, 1, (nq, dim))
    with ScanIndex(dim, 32, metric, devices=[0]) as ix:
        for name, val in [("sketch", 1), ("sketch_min_rows", 1), ("multi_query", 0), ("radius_mq", 0), ("sketch_radius", 1),
                          ("sketch_topk_collect", 1)] + opts:
            ix.set_option(name, int(val))
        ix.synth(n, 1234)
        radii = np.ascontiguousarray(ix.search_topk(Q, 25)[1][:, 24])
        calls = {"radius": lambda: ix.search_radius_batch(Q, radii), "k=100": lambda: ix.search_topk(Q, 100)}
        for mode, call in calls.items():
            digest = answer_hash(mode, call())
            ms, wall = [], []
            while len(ms) < 200 and (len(ms) < reps or sum(ms) < min_ms):
                ix.set_timing(True); ix.reset_stats()
                t0 = time.perf_counter(); call(); wall.append(1e3 * (time.perf_counter() - t0))
                s = ix.stats(); ix.set_timing(False)
                ms.append(s["scan_ms"])
            settled = s["sketch_radius_queries"] if mode == "radius" else ix.sketch_topk_stats()["queries"]
            print("%-8s %7d x %4d m%d %-6s nq %4d %-14s: sweeps %9.3f ms best %9.3f median %9.3f worst of %3d  %7.1f passes %4d launches"
                  "  %9.0f queries/s  wall %9.2f ms best  settled %d  answer %s" % (
                      tag, n, dim, metric, mode, nq, os.environ.get("SZG_OPTS", ""), min(ms), sorted(ms)[len(ms) // 2], max(ms), len(ms),
                      s["scan_bytes"] / float(n * dim), s["scan_launches"], 1e3 * nq / min(ms), min(wall), settled, digest), flush=True)
