"""From "new filter text on a string field" to "mask ready", in one process on one card, for a field whose value is
distinct per row ("user%07d@example%d.com", about 25 bytes), through two paths:

  (a) the "string" kind of Collection.IndexField: a SZG_COL_U32 column of codes of a dictionary the host owns -- here as
      many entries as rows -- so a new constant is a Python loop over the dictionary (as Collection._leaf_mask does)
      and szg_mask_where_u32 with the bitmap over codes;
  (b) a text column (SZG_COL_STR): szg_mask_where_str compares the bytes on the card.

    python scripts/dev_where_text.py [--rows 1000000] [--repeats 20] [--out profiles/columns_where_text.txt]

The two legs alternate call by call in the same run, CONTAINS, ENDS_WITH, == and < each; every call uses a constant
that was not used before and its count is checked against the other leg's.  Each timing is a host clock around a call
that ends in a device synchronise; every shape is warmed up first and the median of the repeats is reported with their
spread.  The kernel's own time comes from scripts/where_kernel/where_text_kernel (HIP events, 50 launches after 5
warm-up, against the bytes it must read; see its header for the build line) when that program has been built; without
it the figure is reported as "not measured".  The vectors are dim 8, 8-bit: the kernel does not read them.  One JSON
line per measurement.
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

from syzgydb_amd import ScanIndex  # noqa: E402
from syzgydb_amd.where import Cmp, StrOp  # noqa: E402


def spread(samples):
    return {"median_ms": statistics.median(samples) * 1e3, "min_ms": min(samples) * 1e3, "max_ms": max(samples) * 1e3,
            "repeats": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.rows
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    strings = ["user%07d@example%d.com" % ((i * 2654435761) % 10000000, i % 97) for i in range(n)]
    codes = {}
    for s in strings:
        codes.setdefault(s, len(codes))
    legs = [("CONTAINS", lambda i: StrOp("f", "CONTAINS", "%03d@example" % i)),
            ("ENDS_WITH", lambda i: StrOp("f", "ENDS_WITH", "@example%d.com" % i)),
            ("==", lambda i: Cmp("f", "==", strings[(7919 * i) % n])),
            ("<", lambda i: Cmp("f", "<", "user%07d" % (1000 * i + 500)))]
    with ScanIndex(8, 8, 1, devices=[0]) as ix:
        ix.synth(n, 7)
        t0 = time.perf_counter()
        text = ix.text_column(strings)
        t1 = time.perf_counter()
        coded = ix.column(np.array([codes[s] for s in strings], dtype=np.uint32))
        emit(path="create", rows=n, distinct=len(codes), heap_bytes=sum(len(s) for s in strings),
             text_column_ms=(t1 - t0) * 1e3)

        def dictionary(e):   # Collection._leaf_mask for the "string" kind
            return coded.codes([e.test(s) for s in codes])

        def card(e):
            if isinstance(e, StrOp):
                return {"CONTAINS": text.contains, "ENDS_WITH": text.endswith}[e.op](e.constant)
            return text.where(e.op, e.constant)

        for name, make in legs:
            for i in range(2):   # warm-up, both legs
                dictionary(make(1000 + i)).close()
                card(make(1000 + i)).close()
            ta, tb = [], []
            for i in range(args.repeats):
                e = make(i)
                t0 = time.perf_counter()
                ma = dictionary(e)
                t1 = time.perf_counter()
                mb = card(e)
                t2 = time.perf_counter()
                assert ma.count == mb.count and (ma.read() == mb.read()).all(), e.text()
                ma.close()
                mb.close()
                ta.append(t1 - t0), tb.append(t2 - t1)
            emit(path="a: Python loop over the dictionary + szg_mask_where_u32", op=name, rows=n, **spread(ta))
            emit(path="b: szg_mask_where_str", op=name, rows=n, **spread(tb))
    exe = os.path.join(ROOT, "scripts", "where_kernel", "where_text_kernel")
    if os.path.exists(exe) and n <= 9999999:
        out = subprocess.run([exe, str(n), "50"], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise SystemExit("where_text_kernel failed: %s %s" % (out.stdout, out.stderr))
        for ln in out.stdout.strip().splitlines():
            emit(path="kernel: HIP events", **json.loads(ln))
    else:
        emit(path="kernel: HIP events", rows=n,
             ms_per_launch="not measured (scripts/where_kernel/where_text_kernel is not built)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
