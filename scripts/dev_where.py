"""From "new predicate" to "mask ready", in one process on one card, through two paths:

  (a) the host path every new filter text took before the resident columns: the Python callable once per row over the
      metadata (as Collection._mask_entry does), pack_allow_bits, szg_mask_create;
  (b) szg_mask_where_f64 on a resident column.

    python scripts/dev_where.py [--rows 1000000] [--dim 768] [--bits 32] [--repeats 20] [--host-rows 1000000]
                                [--out results/dev_where.json]

Each timing is a host clock around a call that ends in a device synchronise (both paths download or upload words
synchronously); every shape is warmed up first and the median of the repeats is reported with their spread.  Every
repeat uses a constant that was not used before: a new predicate, as a REST filter carries one.  The compare kernel's
own time comes from scripts/where_kernel/where_kernel (HIP events, see its header for the build line) when that
program has been built; without it the figure is reported as "not measured".  One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from syzgydb_amd import ScanIndex, pack_allow_bits  # noqa: E402


def spread(samples):
    return {"median_ms": statistics.median(samples) * 1e3, "min_ms": min(samples) * 1e3, "max_ms": max(samples) * 1e3,
            "repeats": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--bits", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-rows", type=int, default=1000000, help="rows path (a) is timed at (0: skip it)")
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.rows
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    rng = np.random.default_rng(1)
    price = np.round(rng.uniform(0, 100, n), 2)
    with ScanIndex(args.dim, args.bits, 1, devices=[0]) as ix:
        ix.synth(n, 7)
        col = ix.column(price)
        # (b) the column path
        for i in range(3):
            col.where("<", 1.0 + i).close()
        t = []
        for i in range(args.repeats):
            c = 37.5 + 0.25 * i
            t0 = time.perf_counter()
            m = col.where("<", c)
            t.append(time.perf_counter() - t0)
            assert m.count == int((price < c).sum())
            m.close()
        emit(path="b: szg_mask_where_f64", rows=n, **spread(t))
        base = col.where(">=", 10.0)
        t = []
        for i in range(args.repeats):
            t0 = time.perf_counter()
            m = col.where("<", 40.0 + i, base=base)
            t.append(time.perf_counter() - t0)
            m.close()
        emit(path="b: szg_mask_where_f64 with a base mask", rows=n, **spread(t))
        # (a) the host path, at host_rows rows of the same column (its cost is linear in the rows)
        hn = min(args.host_rows, n)
        if hn:
            meta = [b'{"price": %.2f, "name": "doc"}' % p for p in price[:hn]]
            t_eval, t_pack, t_up = [], [], []
            with ScanIndex(8, 8, 1, devices=[0]) as hx:
                hx.synth(hn, 7)
                hx.mask(np.ones(hn, bool)).close()
                for i in range(args.host_repeats):
                    c = 37.5 + 0.25 * i
                    flt = lambda id_, m, c=c: json.loads(m).get("price", 1e300) < c   # noqa: E731
                    t0 = time.perf_counter()
                    verdicts = np.zeros(hn, dtype=bool)
                    for row in range(hn):
                        verdicts[row] = bool(flt(row, meta[row]))
                    t1 = time.perf_counter()
                    words = pack_allow_bits(verdicts)
                    t2 = time.perf_counter()
                    m = hx.mask(words)
                    t3 = time.perf_counter()
                    assert m.count == int((price[:hn] < c).sum())
                    m.close()
                    t_eval.append(t1 - t0), t_pack.append(t2 - t1), t_up.append(t3 - t2)
            emit(path="a: host callable per row + pack_allow_bits + szg_mask_create", rows=hn,
                 **spread([a + b + c for a, b, c in zip(t_eval, t_pack, t_up)]),
                 callable_median_ms=statistics.median(t_eval) * 1e3, pack_median_ms=statistics.median(t_pack) * 1e3,
                 create_median_ms=statistics.median(t_up) * 1e3)
    exe = os.path.join(ROOT, "scripts", "where_kernel", "where_kernel")
    if os.path.exists(exe):
        out = subprocess.run([exe, str(n), "50"], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise SystemExit("where_kernel failed: %s %s" % (out.stdout, out.stderr))
        emit(path="kernel: HIP events", **json.loads(out.stdout.strip().splitlines()[-1]))
    else:
        emit(path="kernel: HIP events", rows=n, ms_per_launch="not measured (scripts/where_kernel/where_kernel is not built)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
