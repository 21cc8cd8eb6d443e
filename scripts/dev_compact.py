"""Compaction on the card against the only route there was before it, the round trip through the host.

Per case (1M x 768 float32 cosine with 10 % and 50 % seeded tombstones, 1M x 768 8-bit, tiled, with 10 %), in one
process on one box, one warm-up and the median of 5 each:
  compact()      ScanIndex.compact(): wall time of the call (it synchronises the device before it returns), and the
                 rate of its row gather as read + write bytes of the kept rows over that time
  host route     read_rows -> numpy select -> load (the tombstones themselves are not needed for it: it moves the
                 same bytes with or without them, so its repeats skip the tombstone calls)
  searches       a lone search_topk and a 16-query multi_query = 0 call, median of 20 each, with the tombstones in
                 place, after compaction, and on a never-tombstoned index of as many rows as were kept
SZG_ROWS (1000000) and SZG_REPS (5) shrink it for a rehearsal."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syzgydb_amd import ScanIndex  # noqa: E402
from syzgydb_amd.synth import synth_vectors  # noqa: E402

N = int(os.environ.get("SZG_ROWS", "1000000"))
REPS = int(os.environ.get("SZG_REPS", "5"))
DIM, K = 768, 10
COPY_PEAK = 6.29e12   # bytes/s a plain copy kernel reaches on this card (read + write counted)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def search_times(ix, Q):
    out = []
    for q in (Q[:1], Q[:16]):
        for _ in range(3):
            ix.search_topk(q, K)
        out.append(median([timed(lambda: ix.search_topk(q, K)) for _ in range(20)]))
    return out


def case(bits, frac):
    dead = np.random.default_rng(bits * 100 + int(frac * 100)).choice(N, int(N * frac), replace=False)
    Q = synth_vectors(99, 0, 16, DIM)
    with ScanIndex(DIM, bits, 1, devices=[0]) as ix:
        ix.set_option("multi_query", 0)
        pitch = (ix.row_bytes + 15) // 16 * 16
        kept = N - len(dead)
        compact_ms, host_ms, before, after = [], [], None, None
        for rep in range(REPS + 1):   # (rep 0 warms up)
            ix.synth(N, 1234)
            for r in dead:
                ix.tombstone(int(r))
            if rep == REPS:
                before = search_times(ix, Q)
            ms = timed(ix.compact)
            assert ix.rows == ix.live_rows == kept
            if rep:
                compact_ms.append(ms)
            print("  rep %d compact %.2f ms" % (rep, ms), flush=True)
        after = search_times(ix, Q)
        live = np.ones(N, bool)
        live[dead] = False
        for rep in range(REPS + 1):
            ix.synth(N, 1234)

            def route():
                data = ix.read_rows(0, ix.rows)
                ix.load(data[live])
            ms = timed(route)
            assert ix.rows == kept
            if rep:
                host_ms.append(ms)
            print("  rep %d host route %.0f ms" % (rep, ms), flush=True)
        ix.synth(kept, 1234)
        fresh = search_times(ix, Q)
    c, h = median(compact_ms), median(host_ms)
    rate = 2.0 * kept * pitch / (c * 1e-3)
    print("%2d-bit x %d, %d rows, %2.0f %% tombstoned: compact %.2f ms (%.2f TB/s read + write = %.2f of a copy "
          "pass), host route %.0f ms (x %.0f); lone search %.3f -> %.3f ms (never tombstoned: %.3f), 16 queries "
          "%.3f -> %.3f ms (%.3f)" % (
              bits, DIM, N, 100 * frac, c, rate / 1e12, rate / COPY_PEAK, h, h / c, before[0], after[0], fresh[0],
              before[1], after[1], fresh[1]), flush=True)


if __name__ == "__main__":
    for bits, frac in ((32, 0.10), (32, 0.50), (8, 0.10)):
        case(bits, frac)
