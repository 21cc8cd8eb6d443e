"""Option query_prep (a sketch batch's queries prepared on the card): what one call of n queries costs with the option
at SZG_QP (0, 1 or 2; default 0 -- the setting an older build selected through SZG_LIB_PATH can run), and the kernel
alone for a profiler.

  SZG_QP=2 python scripts/dev_query_prep.py calls     one call of n = 1, 2, 4, 8, 16, 32, 64, 1024 queries, SZG_REPS (30)
                                                      times each after warm-ups: min / median / max wall in microseconds, and
                                                      the host's prepare / enqueue / assemble per query (szg_stats)
  python scripts/dev_query_prep.py kernel             launches of the preparing kernel alone, through the debug hook, for
                                                      4, 32 and 64 queries (under rocprofv3 --kernel-trace --stats: the
                                                      kernel's time per launch size is in the trace)
SZG_ROWS x SZG_DIM float32 cosine (SZG_METRIC), k = 10, multi_query = 0 so that every count goes through the sketch."""
import os, sys, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syzgydb_amd import ScanIndex
from syzgydb_amd.synth import synth_vectors
n, dim, k = int(os.environ.get('SZG_ROWS', '1000000')), int(os.environ.get('SZG_DIM', '768')), 10
metric = int(os.environ.get('SZG_METRIC', '1'))
reps = int(os.environ.get('SZG_REPS', '30'))
qp = int(os.environ.get('SZG_QP', '0'))
mode = sys.argv[1] if len(sys.argv) > 1 else 'calls'
q = synth_vectors(99, 0, 1024, dim)
with ScanIndex(dim, 32, metric, devices=[0]) as ix:
    ix.synth(n, 1234)
    ix.set_option("sketch", 1); ix.set_option("multi_query", 0)
    if qp: ix.set_option("query_prep", qp)
    ix.search_topk(q[:128], k)
    if mode == 'kernel':
        for nq in (4, 32, 64):
            for i in range(20): ix.debug_query_prep(q[:nq], 1)
        print("kernel launches done: 20 each of 4, 32 and 64 queries", flush=True)
        sys.exit(0)
    for nq in (1, 2, 4, 8, 16, 32, 64, 1024):
        r = reps if nq < 1024 else max(5, reps // 5)
        for i in range(5): ix.search_topk(q[:nq], k)
        ix.reset_stats()
        walls = []
        for i in range(r):
            t0 = time.perf_counter(); ix.search_topk(q[:nq], k); walls.append((time.perf_counter() - t0) * 1e6)
        s = ix.stats()
        side = ix.query_prep_stats() if hasattr(ix._L, "szg_index_query_prep_stats") else {}
        print("query_prep=%d n=%-4d wall us min %.1f median %.1f max %.1f | host us per query: prepare %.2f enqueue %.2f assemble %.2f | "
              "settled %d of %d %s" % (qp, nq, min(walls), statistics.median(walls), max(walls), s["host_prep_us"] / (r * nq),
                                       s["host_enqueue_us"] / (r * nq), s["host_finish_us"] / (r * nq), s["sketch_queries"], r * nq,
                                       side), flush=True)
