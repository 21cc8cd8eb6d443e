"""A compaction of a Collection with indexed fields, in one process on one card, through two routes:

  (a) the route before columns were carried: ScanIndex.compact() renumbers the rows, every column goes stale, and
      Collection._rebuild_columns() parses the resident metadata again (json.loads per document), rebuilds every
      indexed field and the hidden object column, and uploads them;
  (b) ScanIndex.compact(carry=columns): the columns follow their rows on the card (Collection.Compact as it stands).

    python scripts/dev_compact_columns.py [--rows 1000000] [--repeats 5] [--out profiles/columns_carry.txt]

1M rows (dim 8, 8-bit: nothing here reads the vectors) with a number field, a string field of five distinct values and
a text field that is distinct per row ("user%07d@example%d.com", 24.9 MB), 10 % and 50 % of the rows tombstoned.  The
legs alternate call by call; before each call the collection is put back (rows loaded, columns rebuilt, tombstones
set), which is not timed.  A timing is a host clock around the whole call, the host's bookkeeping of ids and metadata
included in both legs; one warm-up call per leg, then the median of the repeats with their spread.  After every call
all four columns are read back and compared between the legs.  The carry's kernels alone come from
scripts/carry_kernel/carry_kernel (HIP events, against the bytes they must move and the 6.29 TB/s a copy pass reaches,
DESIGN.md section 6; see its header for the build line) when that program has been built.  One JSON line per
measurement.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from syzgydb_amd import Collection, CollectionOptions  # noqa: E402

COPY_TBS = 6.29   # a plain copy kernel on this card ("Compaction on the card")


def spread(samples):
    return {"median_ms": statistics.median(samples) * 1e3, "min_ms": min(samples) * 1e3, "max_ms": max(samples) * 1e3,
            "repeats": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.rows
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    brands = ["acme", "globex", "initech", "umbrella", "hooli"]
    metas = [('{"price": %s, "brand": "%s", "email": "user%07d@example%d.com"}'
              % ((i % 2000) * 0.5, brands[i % 5], (i * 2654435761) % 10000000, i % 97)).encode() for i in range(n)]
    ids = list(range(n))
    c = Collection(CollectionOptions(Name="carry", DistanceMethod=1, DimensionCount=8, Quantization=8), devices=[0],
                   strict_order=False)
    c._index.synth(n, 7)
    rows = c._index.read_rows(0, n)
    c._id_of, c._meta, c._row_of = list(ids), list(metas), {i: i for i in ids}
    for name, kind in (("price", "number"), ("brand", "string"), ("email", "text")):
        c.IndexField(name, kind)
    emit(path="setup", rows=n, text_heap_bytes=c._fields["email"].column.info()["heap_used"])

    def put_back(share):
        """The collection as before the compaction: n rows, fresh columns, every k-th row tombstoned."""
        c._index.load(rows)
        c._id_of, c._meta, c._row_of = list(ids), list(metas), {i: i for i in ids}
        c._rebuild_columns()
        step = round(1 / share)
        for row in range(0, n, step):
            c._index.tombstone(row)
            del c._row_of[row]
            c._id_of[row], c._meta[row] = None, b""
            # (removeDocument also marks the row absent in every column: dropped rows, the same in both legs)
        return n // step + (n % step > 0)

    def leg_a():
        carried = c._resident_columns
        c._resident_columns = lambda: []   # ScanIndex.compact() without columns: they all go stale
        try:
            c.Compact()
        finally:
            c._resident_columns = carried
        c._rebuild_columns()

    def leg_b():
        c.Compact()

    def reads():
        cols = [c._fields["price"].column, c._fields["brand"].column, c._fields["email"].column, c._object_col]
        return [col.read() for col in cols], dict(c._fields["brand"].codes)

    def same(a, b):
        (ra, da), (rb, db) = a, b
        assert da == db
        for (va, pa), (vb, pb) in zip(ra, rb):
            assert (pa == pb).all()
            if isinstance(va, list):
                assert all(x == y for x, y, p in zip(va, vb, pa) if p)
            else:
                assert (va[pa] == vb[pb]).all()

    for share in (0.1, 0.5):
        ta, tb = [], []
        for i in range(args.repeats + 1):   # call 0 warms both legs up
            got = []
            for leg, samples in ((leg_a, ta), (leg_b, tb)):
                dropped = put_back(share)
                rebuilds = c.column_rebuilds
                t0 = time.perf_counter()
                leg()
                t1 = time.perf_counter()
                assert c._index.rows == n - dropped
                assert c.column_rebuilds == rebuilds + (leg is leg_a)
                if i:
                    samples.append(t1 - t0)
                got.append(reads())
            same(got[0], got[1])
            emit(path="call", tombstoned=share, call=i, a_ms=(ta[-1] if i else None) and ta[-1] * 1e3,
                 b_ms=(tb[-1] if i else None) and tb[-1] * 1e3, reads_equal=True)
        emit(path="a: compact() + _rebuild_columns()", rows=n, tombstoned=share, **spread(ta))
        emit(path="b: compact(carry=columns)", rows=n, tombstoned=share, **spread(tb),
             ratio_a_over_b=statistics.median(ta) / statistics.median(tb))
    c.Close()
    exe = os.path.join(ROOT, "scripts", "carry_kernel", "carry_kernel")
    for percent in (10, 50):
        if os.path.exists(exe) and n <= 9999999:
            out = subprocess.run([exe, str(n), str(percent), "20"], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("carry_kernel failed: %s %s" % (out.stdout, out.stderr))
            for ln in out.stdout.strip().splitlines():
                k = json.loads(ln)
                emit(path="kernels: HIP events", tombstoned=percent / 100, **k,
                     share_of_copy_pass=k["gb_per_s"] / (COPY_TBS * 1e3))
        else:
            emit(path="kernels: HIP events", rows=n, tombstoned=percent / 100,
                 ms_per_carry="not measured (scripts/carry_kernel/carry_kernel is not built)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
