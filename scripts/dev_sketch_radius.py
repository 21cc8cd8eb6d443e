"""Radius searches through the 8-bit sketch (option sketch_radius) against the float32 sweeps they replace: SZG_ROWS
(1000000) x SZG_DIM (768) float32 rows, cosine, radii at each query's SZG_HITS-th (300) neighbour.

Legs, alternated round by round in ONE process (SZG_ROUNDS timed regions each, 7; the median, min and max are printed):
  lone       szg_search_radius, one call per query        float32 sweep | sketch_radius = 1
  call<nq>   one call of nq queries with radius_mq = 0    float32 sweeps | sketch, one-query collect sweeps
             (nq = 16 and 64)                             (sketch_matrix = 1) | the matrix collect form | sketch_wide = 2
  shared     the same queries as a default-option batch   (radius_mq = 1: one shared sweep), for context
Per leg: wall per call, the sweeps' own time per call (HIP events around the scan launches, szg_stats.scan_ms), the bytes
swept per call, hits and -- from the certificate trace of one untimed call -- candidates re-ranked per hit.
A library from before the option (SZG_LIB_PATH, for the A/B against the parent commit) runs the float32 legs only."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from syzgydb_amd import ScanIndex, SzgError, _lib
from syzgydb_amd.synth import synth_vectors

dim, n = int(os.environ.get("SZG_DIM", "768")), int(os.environ.get("SZG_ROWS", "1000000"))
rounds, hits_at = int(os.environ.get("SZG_ROUNDS", "7")), int(os.environ.get("SZG_HITS", "300"))
tag = os.environ.get("SZG_TAG", "tree")
Q = synth_vectors(7, 0, 64, dim)


def leg_options(ix, opts):
    for name, val in opts.items():
        ix.set_option(name, val)


def region(ix, call, reps):
    ix.reset_stats()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = call()
    wall = 1e3 * (time.perf_counter() - t0) / reps   # (every call ends in its own synchronise: the answer is on the host)
    s = ix.stats()
    return wall, s["scan_ms"] / reps, s["scan_bytes"] / reps, out, s


with ScanIndex(dim, 32, 1, devices=[0]) as ix:
    ix.synth(n, 1234)
    have = True
    try:
        ix.set_option("sketch_radius", 0)
    except SzgError:
        have = False
    _, d, _ = ix.search_topk(Q, hits_at)
    radii = np.ascontiguousarray(d[:, -1]) * (1.0 + 1e-9)
    sk = {"sketch": 1, "sketch_min_rows": 1, "sketch_radius": 1}
    off = {"sketch_radius": 0} if have else {}
    legs = [("lone float32", dict(off), "lone", 1)]
    if have:
        legs += [("lone sketch", dict(sk), "lone", 1)]
    for nq in (16, 64):
        legs += [("call%d float32" % nq, dict(off, radius_mq=0), "call", nq)]
        if have:
            legs += [("call%d sketch one-query" % nq, dict(sk, radius_mq=0, sketch_matrix=1, sketch_wide=1), "call", nq),
                     ("call%d sketch matrix" % nq, dict(sk, radius_mq=0, sketch_matrix=0, sketch_wide=1), "call", nq)]
            if nq > 16:
                legs += [("call%d sketch wide" % nq, dict(sk, radius_mq=0, sketch_matrix=0, sketch_wide=2), "call", nq)]
    legs += [("shared64 default batch", dict(off, radius_mq=1), "call", 64)]

    def runner(kind, nq):
        if kind == "lone":
            return (lambda: [ix.search_radius(Q[i], float(radii[i])) for i in range(8)]), 8
        return (lambda: ix.search_radius_batch(Q[:nq], radii[:nq])), 1

    ix.set_timing(True)
    seen = {name: [] for name, _, _, _ in legs}
    extra = {}
    for rnd in range(rounds + 1):   # round 0 warms every leg up
        for name, opts, kind, nq in legs:
            leg_options(ix, opts)
            call, per = runner(kind, nq)
            reps = max(1, (40 if kind == "lone" else 160 // nq) // (4 if rnd == 0 else 1))
            wall, scan, nbytes, out, s = region(ix, call, reps)
            if rnd:
                seen[name].append((wall / per, scan / per, nbytes / per))
                extra[name][:3] = [sum(len(r) for r, _ in out) / len(out), s.get("sketch_radius_queries", 0) // reps,
                                   s.get("sketch_radius_fallbacks", 0) // reps]
            else:
                extra[name] = [0.0, 0, 0, float("nan")]
                if opts.get("sketch_radius"):   # candidates re-ranked per hit: the trace of one untimed call
                    call()   # (the buffers have grown to what these queries collect)
                    ix.trace_certificates(True)
                    out = call()
                    recs, ents, _ = ix.certificates()
                    ix.trace_certificates(False)
                    own = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH_RADIUS]
                    got = sum(len(r) for r, _ in out[:len(own)]) if len(own) else 0
                    extra[name][3] = float(own["n_entries"].sum()) / max(got, 1)
            if have:
                leg_options(ix, {"sketch": 2, "sketch_min_rows": 4096, "sketch_matrix": 0, "sketch_wide": 0, "radius_mq": 1})
    print("# %s: %d x %d float32 cosine, radii at neighbour %d, %d regions per leg (median [min .. max])" % (tag, n, dim, hits_at, rounds))
    for name, _, kind, nq in legs:
        a = np.array(seen[name])
        med, lo, hi = np.median(a, axis=0), a.min(axis=0), a.max(axis=0)
        unit = "query" if kind == "lone" else "call"
        print("%-4s %-26s wall %8.3f ms/%s [%7.3f .. %7.3f]  sweeps %8.3f ms [%7.3f .. %7.3f]  %7.3f GB swept  hits/query %6.0f  "
              "settled %d handed over %d per call  candidates/hit %.2f" % (
                  tag, name, med[0], unit, lo[0], hi[0], med[1], lo[1], hi[1], med[2] / 1e9, extra[name][0],
                  extra[name][1], extra[name][2], extra[name][3]), flush=True)
