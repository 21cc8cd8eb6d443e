"""Top-k searches on float64 rows (the reference's default quantization) through the 8-bit sketch (option sketch_f64 = 1)
against the handle's own sweeps (sketch_f64 = 0, the path of a library without the option): SZG_ROWS (1000000) x SZG_DIM
(768) 64-bit rows, cosine and Euclid, k = 10, multi_query = 0 (each query of a call takes a sweep of its own -- a default-
option batch shares one sweep on the matrix cores and never goes through the sketch, with or without the option; it is
measured once for context).

Legs, alternated round by round on ONE handle in ONE process (SZG_ROUNDS timed regions each, 5; median [min .. max]):
  lone        one query per call                       sketch_f64 = 0 | sketch_f64 = 1
  call1024    one call of SZG_QUERIES (1024) queries   sketch_f64 = 0 | sketch_f64 = 1
  shared      the same call under multi_query = 1      (context)
Per leg: wall per call, the bytes swept per call (szg_stats.scan_bytes), queries settled and handed over per call.
Before the legs: device memory before and after the first sync, the time of the full sketch build (the first search less
a later one), and the same for a float32 handle of the same shape, which reads half the bytes."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from syzgydb_amd import ScanIndex
from syzgydb_amd.synth import synth_vectors

dim, n = int(os.environ.get("SZG_DIM", "768")), int(os.environ.get("SZG_ROWS", "1000000"))
rounds, nq_call = int(os.environ.get("SZG_ROUNDS", "5")), int(os.environ.get("SZG_QUERIES", "1024"))
k = 10
Q = synth_vectors(7, 0, nq_call, dim) * 0.7


def free_bytes():
    """hipMemGetInfo of device 0, from the runtime the library itself has loaded."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    if hip.hipSetDevice(0) != 0 or hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        return float("nan")
    return free.value


def build_time(bits, metric, opts):
    """-> (ms of the full build, bytes the sketch index took, the open handle)"""
    ix = ScanIndex(dim, bits, metric, devices=[0])
    ix.synth(n, 1234)
    for name, val in opts.items():
        ix.set_option(name, val)
    ix.search_topk(Q[:1], k)           # contexts, buffers, the kernels' first launch: everything but the sketch
    before = free_bytes()
    ix.set_option("sketch", 1)
    t0 = time.perf_counter()
    ix.search_topk(Q[:1], k)           # sync: scale pass (Euclid), full build; then the search
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    ix.search_topk(Q[:1], k)
    again = time.perf_counter() - t0
    info = ix.sketch_info()
    assert info["exists"] == 1 and info["in_sync"] == 1 and info["rows"] == n, info
    return 1e3 * (first - again), before - free_bytes(), ix


def region(ix, call, reps):
    ix.reset_stats()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    wall = 1e3 * (time.perf_counter() - t0) / reps
    s = ix.stats()
    return wall, s["scan_bytes"] / reps, s["sketch_queries"] / reps, s["sketch_fallbacks"] / reps


for metric, mname in ((1, "cosine"), (0, "euclid")):
    base = {"sketch": 0, "sketch_min_rows": 1, "multi_query": 0}
    ms32, mem32, ix32 = build_time(32, metric, base)
    ix32.close()
    ms64, mem64, ix = build_time(64, metric, dict(base, sketch_f64=1))
    print("# %d x %d %s: full sketch build  float64 rows %8.1f ms (+%.3f GB device memory over %.3f GB of rows)  "
          "float32 rows %8.1f ms (+%.3f GB over %.3f GB)" % (n, dim, mname, ms64, mem64 / 1e9, n * dim * 8 / 1e9, ms32,
                                                              mem32 / 1e9, n * dim * 4 / 1e9), flush=True)
    legs = [("lone sketch_f64=0", {"sketch_f64": 0, "multi_query": 0}, 1), ("lone sketch_f64=1", {"sketch_f64": 1, "multi_query": 0}, 1),
            ("call%d sketch_f64=0" % nq_call, {"sketch_f64": 0, "multi_query": 0}, nq_call),
            ("call%d sketch_f64=1" % nq_call, {"sketch_f64": 1, "multi_query": 0}, nq_call),
            ("call%d shared sweep" % nq_call, {"sketch_f64": 0, "multi_query": 1}, nq_call)]
    seen = {name: [] for name, _, _ in legs}
    for rnd in range(rounds + 1):   # round 0 warms every leg up
        for name, opts, nq in legs:
            for o, v in opts.items():
                ix.set_option(o, v)
            reps = (20 if nq == 1 else 1) if rnd else 1
            got = region(ix, (lambda: ix.search_topk(Q[:nq], k)), reps)
            if rnd:
                seen[name].append(got)
    for name, _, nq in legs:
        a = np.array(seen[name])
        med, lo, hi = np.median(a, axis=0), a.min(axis=0), a.max(axis=0)
        print("%-6s %-26s wall %9.3f ms/call [%9.3f .. %9.3f]  %9.0f queries/s  %8.3f GB swept  settled %6.1f handed over %5.1f per call" % (
            mname, name, med[0], lo[0], hi[0], nq / med[0] * 1e3, med[1] / 1e9, med[2], med[3]), flush=True)
    ix.close()
