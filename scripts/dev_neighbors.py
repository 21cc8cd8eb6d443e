"""Neighbours of stored rows, in one process on one card: ScanIndex.neighbors (szg_index_neighbors: the sketch-on-sketch
join where it serves) against the route there was -- fetch_into a float64 tensor + search_topk_tensor in calls of 1 024 --
at default options and under query_prep = 1, on a synthetic float32 cosine handle.

    python scripts/dev_neighbors.py [--rows 1000000] [--dim 768] [--queries 64,1024,16384] [--k 10] [--repeats 5]

Each timing is a host clock around the whole call (both routes end with the answers on the host).  The legs alternate call
by call after one warm-up each; medians with their spread; the answers of every pair are compared on their bits.  One
JSON line per query count: times, queries/s, the join's counters (bytes swept per query, the settled share)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from syzgydb_amd import ScanIndex, SZG_COSINE  # noqa: E402


def route(ix, first, n, k, buf):
    ix.fetch_into(buf[:n], first_row=first, n_rows=n)
    out = [ix.search_topk_tensor(buf[i:min(i + 1024, n)], k) for i in range(0, n, 1024)]
    return tuple(np.concatenate([o[j] for o in out]) for j in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", default="64,1024,16384")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dev_neighbors.py needs a GPU: a timing taken without one says nothing")
    counts = [int(x) for x in a.queries.split(",")]
    with ScanIndex(a.dim, 32, SZG_COSINE) as ix:
        ix.synth(a.rows, seed=11)
        ix.debug_join_min_queries(1)   # (the default routes every call past the join: this script measures it)
        buf = torch.empty((max(counts), a.dim), dtype=torch.float64, device="cuda")
        for n in counts:
            legs = {"join": lambda: ix.neighbors(first=0, n=n, k=a.k), "route": lambda: route(ix, 0, n, a.k, buf)}
            times = {name: [] for name in legs}
            got = {}
            for name, f in legs.items():
                got[name] = f()   # warm-up
            same = all((x == y).all() for x, y in zip(got["join"], got["route"]))
            ix.reset_stats()
            for _ in range(a.repeats):
                for name, f in legs.items():
                    t0 = time.perf_counter()
                    f()
                    times[name].append(time.perf_counter() - t0)
            st = ix.neighbors_stats()
            ix.set_option("query_prep", 1)
            route(ix, 0, n, a.k, buf)
            qp = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                route(ix, 0, n, a.k, buf)
                qp.append(time.perf_counter() - t0)
            ix.set_option("query_prep", 0)
            med = {name: statistics.median(v) for name, v in times.items()}
            print(json.dumps({
                "rows": a.rows, "dim": a.dim, "queries": n, "k": a.k, "answers_equal": bool(same),
                "join_ms": med["join"] * 1e3, "join_spread_ms": (max(times["join"]) - min(times["join"])) * 1e3,
                "route_ms": med["route"] * 1e3, "route_spread_ms": (max(times["route"]) - min(times["route"])) * 1e3,
                "route_query_prep_ms": statistics.median(qp) * 1e3,
                "join_queries_per_s": n / med["join"], "route_queries_per_s": n / med["route"],
                "join_bytes_per_query": st["join_bytes"] / max(1, st["join_queries"]),
                "settled_share": 1.0 - st["join_fallbacks"] / max(1, st["join_queries"]), "stats": st}), flush=True)


if __name__ == "__main__":
    main()
