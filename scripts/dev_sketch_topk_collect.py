"""Top-k searches of large k through the 8-bit sketch (option sketch_topk_collect = 1) against the sweeps they replace (the
option at 0: the path of a library without it), on ONE handle per shape in ONE process, the option alternating 0 / 1 over
SZG_REPS (3) repetitions, k = SZG_K (100), multi_query = 0 throughout:

  1M x 768 float32, cosine and Euclid      a lone call, one call of 64 and one of 1 024 queries
  1.25M x 768 float32 Euclid               the cfg4 shard shape: the same three
  1M x 768 float64 cosine, sketch_f64 = 1  the same three

Per leg and option value: wall per call (every call ends with its answer on the host) as min / median / max over the
repetitions, the sweeps' own time per call by HIP events (szg_stats.scan_ms: the float32 sweeps, or the collect sweeps --
the sample pass is not inside that pair), bytes swept per query, and with the option on the queries settled / handed over
and the candidates gathered per query.  The verdict column applies the rule of DESIGN.md 6: a shape stays served only if
its SLOWEST run with the option on beats its FASTEST run with it off.

SZG_SHAPES picks shapes by name (f32cos,f32euc,cfg4,f64cos); SZG_ROWS scales the 1M shapes."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from syzgydb_amd import ScanIndex
from syzgydb_amd.synth import synth_vectors

dim = int(os.environ.get("SZG_DIM", "768"))
rows = int(os.environ.get("SZG_ROWS", "1000000"))
reps = int(os.environ.get("SZG_REPS", "3"))
k = int(os.environ.get("SZG_K", "100"))
names = os.environ.get("SZG_SHAPES", "f32cos,f32euc,cfg4,f64cos").split(",")
SHAPES = {"f32cos": (32, 1, rows), "f32euc": (32, 0, rows), "cfg4": (32, 0, rows * 5 // 4), "f64cos": (64, 1, rows)}
Q = synth_vectors(7, 0, 1024, dim)
LEGS = (("lone", 1, 8), ("call64", 64, 2), ("call1024", 1024, 1))   # name, queries per call, calls per timed region


def region(ix, nq, calls):
    ix.reset_stats()
    t0 = time.perf_counter()
    for c in range(calls):
        ix.search_topk(Q[:nq] if nq > 1 else Q[c], k)
    wall = 1e3 * (time.perf_counter() - t0) / calls
    s, ts = ix.stats(), ix.sketch_topk_stats()
    n = calls * nq
    return wall, s["scan_ms"] / calls, s["scan_bytes"] / n, ts["queries"] / calls, ts["fallbacks"] / calls, \
        ts["candidates"] / max(ts["queries"], 1)


print("# %d x %d (cfg4: %d rows), k = %d, multi_query = 0, %d repetitions per option value, option alternating 0 / 1" % (
    rows, dim, rows * 5 // 4, k, reps))
print("%-7s %-9s %-3s %27s %10s %12s %8s %7s %11s  %s" % ("shape", "leg", "opt", "wall ms/call min med max", "sweeps ms",
                                                           "GB/query", "settled", "handed", "cands/query", "verdict"))
for name in names:
    bits, metric, n = SHAPES[name]
    with ScanIndex(dim, bits, metric, devices=[0]) as ix:
        for opt, val in (("sketch_f64", 1 if bits == 64 else 0), ("sketch", 1), ("sketch_min_rows", 1), ("multi_query", 0)):
            ix.set_option(opt, val)
        ix.synth(n, 1234)
        ix.set_timing(True)
        for leg, nq, calls in LEGS:
            seen = {0: [], 1: []}
            for rep in range(reps + 1):   # repetition 0 warms both values up (the sketch is built, the buffers grow)
                for on in (0, 1):
                    ix.set_option("sketch_topk_collect", on)
                    r = region(ix, nq, calls)
                    if rep:
                        seen[on].append(r)
            a0, a1 = np.array(seen[0]), np.array(seen[1])
            verdict = "stays served" if a1[:, 0].max() < a0[:, 0].min() else "NOT faster: taken out"
            for on, a in ((0, a0), (1, a1)):
                print("%-7s %-9s %-3d %8.3f %8.3f %8.3f %10.3f %12.4f %8.1f %7.1f %11.0f  %s" % (
                    name, leg, on, a[:, 0].min(), np.median(a[:, 0]), a[:, 0].max(), np.median(a[:, 1]), np.median(a[:, 2]) / 1e9,
                    np.median(a[:, 3]), np.median(a[:, 4]), np.median(a[:, 5]), verdict if on else ""), flush=True)
