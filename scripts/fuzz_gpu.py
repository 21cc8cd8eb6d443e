"""Differential fuzzing of the C-ABI search entry points against the CPU oracle.

Random shapes (dim, quantization, metric, rows, k, batch size), filter masks, tombstones,
two-shard handles, duplicate-heavy and scaled corpora, queries at and within a few float32 spacings of stored rows
("coincident", at every row width), random tunables -- the options that are soaking (sketch_radius, sketch_masked,
sketch_f64, sketch_topk_collect) and the sketch sweep's forms among them.  Every answer must be
the oracle's: same rows in the same order, bit-equal float64 distances (NaN == NaN).

    python scripts/fuzz_gpu.py [seconds] [seed] [--iterations N] [--certificates]

--iterations N runs exactly N cases instead of a time budget: a seed then means the same cases on every run.
--certificates switches the handles' certificate trace on and checks every search call's records against float64
(syzgydb_amd/cert_check.py: key bounds, left-out bounds, collect completeness, the sketch's bound) beside the answers;
the cases drawn are the same with and without it.
Dimensions come from a fixed list and from the scan kernel's shape lattice (syzgydb_amd/scan_lattice.py: one dimension per
lane-map class of the drawn row width); about a third of the filtered cases pass their filters as resident masks.
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import oracle as orc
from syzgydb_amd import ScanIndex, cert_check, scan_lattice

ap = argparse.ArgumentParser()
ap.add_argument("seconds", nargs="?", type=float, default=60.0)
ap.add_argument("seed", nargs="?", type=int, default=1)
ap.add_argument("--iterations", type=int, default=0, help="run exactly this many cases (0: run for `seconds`)")
ap.add_argument("--certificates", action="store_true", help="check every call's certificate trace against float64")
args = ap.parse_args()
budget, seed = args.seconds, args.seed
rng = np.random.default_rng(seed)
rng_near = np.random.default_rng([seed, 0x6E656172])   # the coincident queries' own stream: every other draw of a seed stays as it was
rng_more = np.random.default_rng([seed, 0x6D6F7265])   # ... and OPTS_MORE's
DIMS = [1, 2, 3, 5, 16, 17, 31, 32, 33, 64, 100, 128, 129, 384, 500, 768, 1024]
OPTS = [("queries_per_launch", [1, 3, 16]), ("multi_query", [0, 1]), ("force_matrix", [0, 0, 1]),
        ("serialize_scans", [0, 1]), ("mq_min", [2, 8]), ("slack", [0, 16, 40]), ("mq_hits", [64, 1024]),
        ("sketch", [0, 1, 1]), ("sketch_extra", [0, 30]), ("sketch_min_rows", [1, 1, 4096]),
        ("force_no_refine", [0, 0, 1]), ("mask_dense", [0, 1]), ("coalesce", [0, 1]), ("finish_thread", [0, 1, 1]),
        ("radius_mq", [0, 1, 1]), ("query_batch", [5, 16]), ("scan_group", [0, 1, 2, 4]), ("sketch_radius", [0, 1, 1]),
        ("sketch_share", [0, 1, 2, 2]), ("sketch_topk_collect", [0, 1, 1])]
# the options that are soaking and the sketch sweep's forms: drawn from a stream of their own (rng_more), so that every other
# draw of a seed stays what it was before they were added
OPTS_MORE = [("sketch_masked", [0, 1, 1]), ("sketch_f64", [0, 1, 1]), ("sketch_matrix", [0, 1, 2]), ("sketch_select", [0, 1]),
             ("sketch_wide", [0, 1, 2]), ("sketch_bulk", [0, 1, 2]), ("sketch_planes", [0, 3]), ("scan_norms", [0, 1]),
             ("scan_group_ring", [0, 4, 6])]


def same(got_r, got_d, want_r, want_d):
    if len(got_r) != len(want_r):
        return False
    if [int(x) for x in got_r] != [int(x) for x in want_r]:
        return False
    g, w = np.asarray(got_d), np.asarray(want_d)
    return bool(((g == w) | (np.isnan(g) & np.isnan(w))).all())


def certificates(ix, rows, dim, bits, metric, Q, eligible, desc, call, radii=None):
    """--certificates: the records of the call just made, checked; a failed claim counts like a wrong answer."""
    if not args.certificates:
        return 0
    recs, ents, dropped = ix.certificates()
    corpus = cert_check.Corpus(rows, dim, bits, metric)
    Q = np.atleast_2d(Q)
    dists = sketch = None
    if np.isin(recs["pass_"], (1, 5, 6)).any():   # sketch passes, top-k and radius
        dists = np.stack([orc.all_distances(rows, dim, bits, metric, q) for q in Q])
        info = ix.sketch_info()
        if info["exists"] and info["in_sync"]:   # the sketch sweep's own keys and lists too (K_s, L_s, D)
            sketch = (cert_check.Corpus(ix.sketch_rows()[0], dim, 8, metric), info["gscale"], info["exc_rows"])
    try:
        cert_check.check(corpus, Q, recs, ents, dropped, eligible=eligible, dists=dists, what=(call,), sketch=sketch,
                         radii=radii)
        cert_check.check_bf16_tight(corpus, Q, recs, ents, what=(call,))
    except AssertionError as e:
        print("CERTIFICATE", desc, str(e)[:600], flush=True)
        return 1
    return 0


t_end = time.time() + budget
it = fails = 0
while (it < args.iterations) if args.iterations else (time.time() < t_end):
    it += 1
    bits = int(rng.choice([4, 8, 16, 32, 64]))
    metric = int(rng.integers(0, 2))
    dim = int(rng.choice(DIMS + [c.dim for c in scan_lattice.cells(bits)]))
    n = int(rng.choice([1, 2, 15, 16, 17, 63, 64, 65, 200, 1000, 3000, 5000, 9000]))
    if dim * n > 4_000_000:
        n = max(1, 4_000_000 // dim)
    nq = int(rng.choice([1, 2, 7, 8, 9, 16, 17, 33, 50]))
    if rng.random() < 0.04 and dim * n <= 400_000:   # a long call: 3+ shared-sweep batches (the finisher thread)
        nq = int(rng.choice([200, 330]))
    k = int(rng.choice([1, 2, 10, 11, 50, 100, 300, 5000]))
    kind = int(rng.integers(0, 8))
    vec = rng.uniform(-1, 1, (n, dim))
    if kind == 1:          # duplicates
        vec[rng.integers(0, n, n // 2)] = vec[0]
    elif kind == 2:        # coarse grid: many equal distances
        vec = np.round(vec * 2) / 2
    elif kind == 3 and bits >= 32:   # large magnitudes / far from the origin
        vec = vec * 1e3 + 5e3
    elif kind == 4:        # some zero rows
        vec[rng.integers(0, n, max(1, n // 10))] = 0.0
    Q = rng.uniform(-1, 1, (nq, dim))
    if kind == 5:          # rows antipodal / parallel to a query among the first rows: the unclamped acos
        for r0 in rng.integers(0, min(n, max(k, 4)), 3):   # (collection.go:831) can return NaN for them, and the
            vec[r0] = Q[0] * float(rng.choice([-0.5, -1.0, 0.5, 1.0]))   # first k rows enter the heap regardless
    elif kind == 6 and bits >= 32:   # NaN / Inf elements in stored rows
        for r0 in rng.integers(0, n, 3):
            vec[r0, int(rng.integers(0, dim))] = float(rng.choice([np.nan, np.inf, -np.inf]))
    elif kind == 7 and bits == 32:   # elements whose squares overflow float32 (finite in the reference's float64)
        for r0 in rng.integers(0, n, 4):
            vec[r0] = vec[r0] * float(rng.choice([1e19, 1e25, 1e37]))
    rows = orc.encode_rows(vec, bits)
    if kind == 3 and bits >= 32:
        Q = Q * 1e3 + 5e3
    if rng.random() < 0.2:
        Q[0] = orc.decode_vector(rows[int(rng.integers(0, n))], dim, bits)   # a stored row as the query
    coincident = rng_near.random() < 0.15   # at every width: queries that round to a stored row, or sit 1, 3 or 17 spacings
    if coincident:                           # off it -- a stored row itself (above) is exact on 32-bit rows; a key of 0 over a
        for qj in range(min(nq, 4)):         # positive real-number key is not
            x = orc.decode_vector(rows[int(rng_near.integers(0, n))], dim, bits)
            if not np.isfinite(x).all():
                continue
            g = x * (65535.0 if bits == 16 else 1.0)   # the spacing of the prepared element, back in the query's units
            sp = np.spacing(np.abs(g).astype(np.float32)).astype(np.float64) / (65535.0 if bits == 16 else 1.0)
            if bits <= 8:
                sp = np.full(dim, np.abs(x).max() / float(rng_near.choice([16000.0, 30000.0, 1000000.0])))   # a quantization step
            move = float(rng_near.choice([0.25, 0.25, 1.0, 3.0, 17.0]))
            at = rng_near.random(dim) < float(rng_near.choice([0.1, 1.0]))
            at[int(rng_near.integers(0, dim))] = True
            step = rng_near.uniform(-1, 1, dim) if move < 1 else rng_near.choice((-1.0, 1.0), dim)
            Q[qj] = x + at * step * move * sp
    if rng.random() < 0.1:
        Q[-1] = 0.0
    allow = None
    if rng.random() < 0.4:
        allow = rng.random((nq, n)) < rng.choice([0.05, 0.5, 0.95])
    resident = allow is not None and rng.random() < 1 / 3   # the filters go up once, as masks on the card
    devices = [0, 0] if rng.random() < 0.25 else [0]
    opts = {name: int(rng.choice(vals)) for name, vals in OPTS if rng.random() < 0.3}
    opts.update({name: int(rng_more.choice(vals)) for name, vals in OPTS_MORE if rng_more.random() < 0.3})
    dead = []
    desc = dict(it=it, bits=bits, metric=metric, dim=dim, n=n, nq=nq, k=k, kind=kind, coincident=coincident, masked=allow is not None,
                resident=resident, devices=devices, opts=opts)
    try:
        with ScanIndex(dim, bits, metric, devices=devices) as ix:
            split = int(rng.integers(1, n)) if (n > 1 and rng.random() < 0.3) else n
            ix.load(rows[:split])
            if split < n:   # the rest arrives through the mutation entry points
                if rng.random() < 0.5:
                    ix.append(rows[split:])
                else:
                    ix.append_vectors(vec[split:])
            if n > 3 and rng.random() < 0.3:   # overwrite a few rows in place
                for r0 in rng.choice(n, size=min(5, n), replace=False):
                    nv = rng.uniform(-1, 1, dim)
                    vec[r0] = nv
                    rows[r0] = orc.encode_rows(nv.reshape(1, -1), bits)[0]
                    ix.overwrite(int(r0), rows[r0])
            assert (ix.read_rows(0, n) == rows).all(), "read_rows != what was written"
            for name, val in opts.items():
                ix.set_option(name, val)
            if args.certificates:
                ix.trace_certificates(True)
            if rng.random() < 0.3 and n > 2:
                dead = [int(x) for x in rng.choice(n, size=max(1, n // 7), replace=False)]
                for r in dead:
                    ix.tombstone(r)
            live = np.ones(n, dtype=bool)
            live[dead] = False
            handles = [ix.mask(allow[qi]) for qi in range(nq)] if resident else None

            def filt(lo, hi):   # the filters of queries [lo, hi) as the searches take them
                if allow is None:
                    return {}
                return dict(masks=handles[lo:hi]) if resident else dict(allow=allow[lo:hi])
            r, d, c = ix.search_topk(Q, k, **filt(0, nq))
            fails += certificates(ix, rows, dim, bits, metric, Q, live if allow is None else (allow & live), desc, "topk")
            for qi in range(nq):
                m = live if allow is None else (live & allow[qi])
                o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, metric, Q[qi], k=k, allow=m.astype(np.uint8))
                if not same(r[qi, : c[qi]], d[qi, : c[qi]], o_rows, o_dist):
                    fails += 1
                    print("MISMATCH topk", desc, "query", qi, flush=True)
                    print("  got ", [int(x) for x in r[qi, : c[qi]]][:12], d[qi, : c[qi]][:6], flush=True)
                    print("  want", [int(x) for x in o_rows][:12], o_dist[:6], flush=True)
                    break
            # one radius search at a result distance
            qi = int(rng.integers(0, nq))
            m = live if allow is None else (live & allow[qi])
            o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, metric, Q[qi], k=min(k, 20), allow=m.astype(np.uint8))
            finite = [x for x in o_dist if x == x and x > 0]
            if finite:
                radius = float(finite[-1])
                rr, dd = ix.search_radius(Q[qi], radius, **filt(qi, qi + 1))
                fails += certificates(ix, rows, dim, bits, metric, Q[qi], m, desc, "radius", radii=radius)
                w_rows, w_dist, _ = orc.search_exact(rows, dim, bits, metric, Q[qi], radius=radius,
                                                     allow=m.astype(np.uint8))
                if not same(rr, dd, w_rows, w_dist):
                    fails += 1
                    print("MISMATCH radius", desc, "query", qi, radius, len(rr), len(w_rows), flush=True)
            # a BATCH of radius searches, each query its own radius (query-major collect launches, szg_search_radius_batch)
            nb_ = min(nq, int(rng.choice([1, 3, 17, 40])))
            radii = []
            for qj in range(nb_):
                mj = live if allow is None else (live & allow[qj])
                od = orc.search_exact(rows, dim, bits, metric, Q[qj], k=int(rng.choice([1, 5, 60])), allow=mj.astype(np.uint8))[1]
                fin = [x for x in od if x == x and x > 0]
                radii.append(float(fin[-1]) if fin else 0.5)
            hits = ix.search_radius_batch(Q[:nb_], radii, **filt(0, nb_))
            fails += certificates(ix, rows, dim, bits, metric, Q[:nb_], live if allow is None else (allow[:nb_] & live), desc,
                                  "radius batch", radii=radii)
            for qj in range(nb_):
                mj = live if allow is None else (live & allow[qj])
                w_r, w_d, _ = orc.search_exact(rows, dim, bits, metric, Q[qj], radius=radii[qj], allow=mj.astype(np.uint8))
                if not same(hits[qj][0], hits[qj][1], w_r, w_d):
                    fails += 1
                    print("MISMATCH radius batch", desc, "query", qj, radii[qj], len(hits[qj][0]), len(w_r), flush=True)
                    break
            # the candidate re-rank primitives: float64 distances for row lists and row pairs
            pick = rng.integers(0, n, min(n, 40)).astype(np.uint64)
            got = ix.distances(Q[0], pick)
            want = orc.all_distances(rows[pick.astype(np.int64)], dim, bits, metric, Q[0])
            if not bool(((got == want) | (np.isnan(got) & np.isnan(want))).all()):
                fails += 1
                print("MISMATCH distances", desc, flush=True)
            pa = rng.integers(0, n, 20).astype(np.uint64)
            pb = rng.integers(0, n, 20).astype(np.uint64)
            got = ix.pair_distances(pa, pb)
            fn = orc.angular if metric == 1 else orc.euclidean
            want = np.array([fn(orc.decode_vector(rows[int(x)], dim, bits), orc.decode_vector(rows[int(y)], dim, bits))
                             for x, y in zip(pa, pb)])
            if not bool(((got == want) | (np.isnan(got) & np.isnan(want))).all()):
                fails += 1
                print("MISMATCH pair_distances", desc, flush=True)
            # a radius search into a buffer that is too small: the best `cap` hits and the true total
            if finite and len(w_rows) > 3:
                cap = int(rng.integers(1, len(w_rows)))
                tr, td, total = ix.search_radius(Q[qi], radius, allow=None if allow is None else allow[qi], capacity=cap)
                fails += certificates(ix, rows, dim, bits, metric, Q[qi], m, desc, "truncated radius", radii=radius)
                if total != len(w_rows) or not same(tr, td, w_rows[:cap], w_dist[:cap]):
                    fails += 1
                    print("MISMATCH truncated radius", desc, cap, total, len(w_rows), flush=True)
            # a second act: mutations AFTER searches (whatever the handle keeps beside the rows -- resident row norms,
            # sketches, liveness words -- has to follow them), then the same questions again
            if n > 3 and allow is None and rng.random() < 0.4:
                for r0 in rng.choice(n, size=min(4, n), replace=False):
                    if r0 in dead:
                        continue
                    nv = rng.uniform(-1, 1, dim) * float(rng.choice([1.0, 0.3, 0.0]))
                    if rng.random() < 0.5:
                        rows[r0] = orc.encode_rows(nv.reshape(1, -1), bits)[0]
                        ix.overwrite(int(r0), rows[r0])
                    else:
                        ix.overwrite_vector(int(r0), nv)
                        rows[r0] = ix.read_rows(int(r0), 1)[0]
                        assert (rows[r0] == orc.encode_rows(nv.reshape(1, -1), bits)[0]).all(), "device quantization differs"
                extra = int(rng.integers(1, 40))
                ev = rng.uniform(-1, 1, (extra, dim))
                erows = orc.encode_rows(ev, bits)
                ix.append(erows)
                rows2 = np.concatenate([rows, erows])
                live2 = np.concatenate([live, np.ones(extra, dtype=bool)])
                r, d, c = ix.search_topk(Q, k)
                fails += certificates(ix, rows2, dim, bits, metric, Q, live2, desc, "topk after mutation")
                for qi in range(nq):
                    o_rows, o_dist, _ = orc.search_exact(rows2, dim, bits, metric, Q[qi], k=k, allow=live2.astype(np.uint8))
                    if not same(r[qi, : c[qi]], d[qi, : c[qi]], o_rows, o_dist):
                        fails += 1
                        print("MISMATCH topk after mutation", desc, "query", qi, flush=True)
                        break
                nb_ = min(nq, 9)
                radii = []
                for qj in range(nb_):
                    od = orc.search_exact(rows2, dim, bits, metric, Q[qj], k=5, allow=live2.astype(np.uint8))[1]
                    fin = [x for x in od if x == x and x > 0]
                    radii.append(float(fin[-1]) if fin else 0.5)
                hits = ix.search_radius_batch(Q[:nb_], radii)
                fails += certificates(ix, rows2, dim, bits, metric, Q[:nb_], live2, desc, "radius batch after mutation", radii=radii)
                for qj in range(nb_):
                    w_r, w_d, _ = orc.search_exact(rows2, dim, bits, metric, Q[qj], radius=radii[qj], allow=live2.astype(np.uint8))
                    if not same(hits[qj][0], hits[qj][1], w_r, w_d):
                        fails += 1
                        print("MISMATCH radius batch after mutation", desc, "query", qj, flush=True)
                        break
    except Exception as e:  # noqa: BLE001
        fails += 1
        print("EXCEPTION", desc, repr(e), flush=True)
    if it % 25 == 0:
        print("iterations %d, failures %d" % (it, fails), flush=True)
print("FUZZ done: %d iterations, %d failures (seed %d)" % (it, fails, seed), flush=True)
sys.exit(1 if fails else 0)
