"""Bulk mutations against the loop of single-row calls, in one process on one card:

  overwrite   10 000 scattered rows rewritten from float64 vectors --
              (a) ScanIndex.overwrite_vector per row (szg_index_overwrite_f64: a device synchronise, a copy, an encode
                  launch and a stream synchronise each), the way before the bulk calls;
              (b) ONE ScanIndex.overwrite_vectors (szg_index_overwrite_rows_f64);
  tombstone   10 000 scattered live rows dropped --
              (a) ScanIndex.tombstone per row (szg_index_tombstone: a device synchronise and an 8-byte copy each);
              (b) ONE ScanIndex.tombstone_rows.

    python scripts/dev_bulk.py [--rows 1000000] [--dim 768] [--listed 10000] [--repeats 5] [--out profiles/bulk_mutations.txt]

A 1M x 768 float32 cosine handle of synthetic rows (no search runs, so no sketch and no norms exist: the plain cost of
the mutation).  Every call of every leg takes its own 10 000 rows of one permutation, so no row is written or dropped
twice; the legs alternate call by call, one warm-up call per leg, then the median of the repeats with their spread.  A
timing is a host clock around the whole leg.  Every overwrite call of either leg gets vectors in host memory that no
earlier call has uploaded from (fresh arrays, all kept alive), so no leg profits from pages the runtime may still hold
pinned.  After each overwrite pair the two legs' rows, written from the same
vectors, are read back at 64 positions spread over the list and compared; after each tombstone pair the live count is
checked.  One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from syzgydb_amd import ScanIndex, SZG_COSINE  # noqa: E402


def spread(samples):
    return {"median_ms": statistics.median(samples) * 1e3, "min_ms": min(samples) * 1e3, "max_ms": max(samples) * 1e3,
            "repeats": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--listed", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dim, m = args.rows, args.dim, args.listed
    calls = args.repeats + 1
    if 4 * calls * m > n:
        raise SystemExit("--rows is too small for %d calls of %d rows per leg" % (calls, m))
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    rng = np.random.default_rng(11)
    sets = rng.permutation(n)[: 4 * calls * m].astype(np.uint64).reshape(4, calls, m)
    kept = []   # every call's vectors stay alive, so no call uploads from host pages an earlier call has used
    with ScanIndex(dim, 32, SZG_COSINE, devices=[0]) as ix:
        ix.synth(n, 7)
        emit(path="setup", rows=n, dim=dim, bits=32, listed=m)
        ta, tb = [], []
        for i in range(calls):   # call 0 warms both legs up
            rows_a, rows_b = sets[0, i], sets[1, i]
            V = rng.standard_normal((m, dim))   # fresh host memory per call, as a re-embedding run hands over
            kept.append(V)
            t0 = time.perf_counter()
            for r, v in zip(rows_a, V):
                ix.overwrite_vector(int(r), v)
            t1a = time.perf_counter()
            W = V.copy()   # (the bulk leg's own pages: the loop has just read V)
            kept.append(W)
            t1 = time.perf_counter()
            ix.overwrite_vectors(rows_b, W)
            t2 = time.perf_counter()
            probe = np.unique(np.linspace(0, m - 1, 64).astype(np.int64))   # (first and last entry included)
            got_a = np.stack([ix.read_rows(int(r), 1)[0] for r in rows_a[probe]])
            got_b = np.stack([ix.read_rows(int(r), 1)[0] for r in rows_b[probe]])
            assert (got_a == got_b).all()
            if i:
                ta.append(t1a - t0)
                tb.append(t2 - t1)
            emit(path="overwrite call", call=i, loop_ms=(t1a - t0) * 1e3, bulk_ms=(t2 - t1) * 1e3, rows_equal=True)
        emit(path="overwrite a: overwrite_vector per row", rows=n, listed=m, **spread(ta))
        emit(path="overwrite b: one overwrite_vectors", rows=n, listed=m, **spread(tb),
             ratio_a_over_b=statistics.median(ta) / statistics.median(tb))
        ta, tb = [], []
        live = n
        for i in range(calls):
            rows_a, rows_b = sets[2, i], sets[3, i]
            t0 = time.perf_counter()
            for r in rows_a:
                ix.tombstone(int(r))
            t1 = time.perf_counter()
            dropped = ix.tombstone_rows(rows_b)
            t2 = time.perf_counter()
            live -= 2 * m
            assert dropped == m and ix.live_rows == live
            if i:
                ta.append(t1 - t0)
                tb.append(t2 - t1)
            emit(path="tombstone call", call=i, loop_ms=(t1 - t0) * 1e3, bulk_ms=(t2 - t1) * 1e3, live_rows=live)
        emit(path="tombstone a: tombstone per row", rows=n, listed=m, **spread(ta))
        emit(path="tombstone b: one tombstone_rows", rows=n, listed=m, **spread(tb),
             ratio_a_over_b=statistics.median(ta) / statistics.median(tb))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
