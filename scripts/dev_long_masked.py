"""Sweep time of MASKED top-k calls through the sketch of a float32 collection of long rows (1 920 .. 4 096 dimensions)
under sketch_masked = 1, for the library selected by SZG_LIB_PATH (A/B of builds: run once per library, alternating, inside
ONE GPU call; dev_long.py is the unmasked sibling).
  python scripts/dev_long_masked.py rows:dim[:metric] ...   SZG_NQS=1024,16 the calls, SZG_REPS=7, SZG_OPTS=name=v,...
Per shape, call size and mask -- none (the yardstick), rand5 (one resident mask, 5 % of the rows at random), runs5 (the same
share in runs of 4 096 rows), tomb1 (one tombstoned row; last: it changes the handle) -- the HIP-event time of the call's
sweeps (szg_stats.scan_ms, best and median), the passes over the sketch rows, the time per pass, the wall time, settled
queries and fallbacks.  SZG_DUMP=dir: the ids and float64 distances of every timed input go to dir/<tag>_<shape>.npz; with
--compare a.npz b.npz the script only checks two such files for equality."""
import contextlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
if sys.argv[1:2] == ["--compare"]:
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files) and a.files, (a.files, b.files)
    for name in a.files:
        assert a[name].tobytes() == b[name].tobytes(), ("outputs differ", name, sys.argv[2:])
    print("equal: %d arrays of %s and %s" % (len(a.files), sys.argv[2], sys.argv[3]))
    sys.exit(0)
from syzgydb_amd import ScanIndex
tag = os.environ.get("SZG_TAG") or os.path.basename(os.environ.get("SZG_LIB_PATH", "tree")).replace("libsyzgy_scan_", "").replace(".so", "")
nqs = [int(x) for x in os.environ.get("SZG_NQS", "1024,16").split(",")]
reps = int(os.environ.get("SZG_REPS", "7"))
for spec in sys.argv[1:]:
    f = [int(x) for x in spec.split(":")]
    n, dim, metric = f[0], f[1], (f[2] if len(f) > 2 else 1)
    rng = np.random.default_rng(99)
    Q = rng.uniform(-1, 1, (max(nqs), dim))
    rand5 = rng.random(n) < 0.05
    runs5 = np.repeat(rng.random(-(-n // 4096)) < 0.05, 4096)[:n]
    runs5[:4096] = True   # (never empty)
    out = {}
    with ScanIndex(dim, 32, metric, devices=[0]) as ix:
        for name, val in [("sketch", 1), ("sketch_min_rows", 1), ("multi_query", 0), ("sketch_masked", 1)] + [x.split("=") for x in os.environ.get("SZG_OPTS", "").split(",") if x]:
            ix.set_option(name, int(val))
        ix.synth(n, 1234)
        for mask in ("none", "rand5", "runs5", "tomb1"):
            if mask == "tomb1":
                ix.tombstone_rows(np.array([n // 3], dtype=np.uint64))
            with (ix.mask(rand5 if mask == "rand5" else runs5) if mask in ("rand5", "runs5") else contextlib.nullcontext()) as m:
                filt = {"masks": m} if m is not None else {}
                for nq in nqs:
                    q = Q[:nq]
                    ix.search_topk(q, 10, **filt); ix.search_topk(q, 10, **filt)
                    ms, wall = [], []
                    for rep in range(reps):
                        ix.set_timing(True); ix.reset_stats()
                        t0 = time.perf_counter(); got = ix.search_topk(q, 10, **filt); wall.append(1e3 * (time.perf_counter() - t0))
                        s = ix.stats(); ix.set_timing(False)
                        ms.append(s["scan_ms"])
                    out["%s_q%d_ids" % (mask, nq)], out["%s_q%d_dist" % (mask, nq)] = got[0], got[1]
                    passes = s["scan_bytes"] / float(n * dim)
                    print("%-8s %8d x %4d m%d %-5s nq %4d: sweeps %8.3f ms best %8.3f median  %6.1f passes %4d launches  %7.1f us/pass  wall %8.2f ms best"
                          "  settled %d fallbacks %d" % (tag, n, dim, metric, mask, nq, min(ms), sorted(ms)[len(ms) // 2], passes, s["scan_launches"],
                                                      1e3 * min(ms) / max(passes, 1), min(wall), s["sketch_queries"], s["sketch_fallbacks"]), flush=True)
    if os.environ.get("SZG_DUMP"):
        os.makedirs(os.environ["SZG_DUMP"], exist_ok=True)
        np.savez(os.path.join(os.environ["SZG_DUMP"], "%s_%dx%d.npz" % (tag, n, dim)), **out)
