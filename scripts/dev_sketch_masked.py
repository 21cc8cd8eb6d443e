"""Masked top-k calls through the 8-bit sketch with the matrix sweep's masked forms (option sketch_masked = 1) against the
one-query kernel they replace (0), in ONE process on one box: SZG_ROWS (1000000) x SZG_DIM (768) float32 rows, cosine,
k = 10, the median of SZG_ROUNDS (5) timed calls per leg after one warm-up call, legs alternated round by round.

Legs (calls of 1 024 queries unless named otherwise):
  shared <rate>    one resident mask for every query at pass rates 0.9, 0.5, 0.05, 0.001
  tombstones 1%    1 % of the rows removed, no filter
  per-query 0.5    64 resident masks at 0.5, cycled over the queries
  q16 / q64 0.001  calls of 16 and 64 queries under one mask at 0.001 (where the selective one-query form may still win)
  unmasked         the headline call, for the A/B against the parent commit (SZG_LIB_PATH runs this leg alone)
Per leg: wall per call, queries/s, the bytes swept per call (szg_stats.scan_bytes) and the masked matrix launches.
A measurement tool, not a test: run every invocation under a time limit of its own and stop at the first that fails."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from syzgydb_amd import ScanIndex, SzgError
from syzgydb_amd.synth import synth_vectors

dim, n = int(os.environ.get("SZG_DIM", "768")), int(os.environ.get("SZG_ROWS", "1000000"))
rounds, k = int(os.environ.get("SZG_ROUNDS", "5")), 10
tag = os.environ.get("SZG_TAG", "tree")
Q = synth_vectors(7, 0, 1024, dim)
rng = np.random.default_rng(11)

with ScanIndex(dim, 32, 1, devices=[0]) as ix:
    ix.synth(n, 1234)
    have = True
    try:
        ix.set_option("sketch_masked", 0)
    except SzgError:
        have = False
    legs = [("unmasked", 1024, None, None)]
    if have:
        for rate in (0.9, 0.5, 0.05, 0.001):
            legs.append(("shared %g" % rate, 1024, ix.mask(rng.random(n) < rate), None))
        per = [ix.mask(rng.random(n) < 0.5) for _ in range(64)]
        legs.append(("per-query 0.5", 1024, [per[i % 64] for i in range(1024)], None))
        sel = ix.mask(rng.random(n) < 0.001)
        legs += [("q16 0.001", 16, sel, None), ("q64 0.001", 64, sel, None)]
        legs.append(("tombstones 1%", 1024, None, np.flatnonzero(rng.random(n) < 0.01)))   # (last: the rows stay removed)

    def call(nq, masks):
        m = masks[:nq] if isinstance(masks, list) else masks
        return ix.search_topk(Q[:nq], k, masks=m) if m is not None else ix.search_topk(Q[:nq], k)

    print("# %s: %d x %d float32 cosine, k = %d, median of %d calls [min .. max]" % (tag, n, dim, k, rounds))
    for name, nq, masks, dead in legs:
        if dead is not None:
            ix.tombstone_rows(dead)
        opts = (0, 1) if have and name != "unmasked" else (None,)
        seen = {o: [] for o in opts}
        info, answers = {}, {}
        for rnd in range(rounds + 1):   # round 0 warms both settings up
            for o in opts:
                if o is not None:
                    ix.set_option("sketch_masked", o)
                ix.reset_stats()
                t0 = time.perf_counter()
                got = call(nq, masks)
                wall = time.perf_counter() - t0
                st = ix.stats()
                if rnd:
                    seen[o].append(wall)
                info[o] = (st["scan_bytes"], st["sketch_queries"], ix.sketch_masked_info()["launches"] if have else 0)
                answers[o] = got
        if len(opts) == 2:
            assert all((a == b).all() for a, b in zip(answers[0], answers[1])), ("answers differ", name)
        for o in opts:
            a = np.array(seen[o])
            print("%-4s %-16s sketch_masked %-4s wall %9.3f ms [%9.3f .. %9.3f]  %9.0f queries/s  %8.3f GB swept  settled %4d of %4d  "
                  "masked launches %d" % (tag, name, o, 1e3 * np.median(a), 1e3 * a.min(), 1e3 * a.max(), nq / np.median(a),
                                          info[o][0] / 1e9, info[o][1], nq, info[o][2]), flush=True)
