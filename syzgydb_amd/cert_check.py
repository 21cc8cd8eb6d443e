"""The certificate trace checked against float64: what tests/test_gpu_certificates.py, scripts/dev_certificates.py and
scripts/fuzz_gpu.py --certificates share.  Test support, like scan_lattice.py: nothing on the search path imports it.

A Corpus decodes the packed rows once (numpy; check_decode compares rows of it with the oracle's decoder) and computes
the real-number key of every (query, row) pair in float64, or in longdouble where numpy has one wider than float64 and
the case is small:

    cosine   -(q . x) / (|q| |x|)
    Euclid   |q - x|^2 in the key's units: times maxInt^2 for rows of 16 bits or fewer (radius_key_threshold)

together with a bound on the reference's own rounding error, which is added to every tolerance (it is 1e-9 of the
narrowest bound checked or less).  check() then asserts, for every record the trace kept of a call:

    K  each candidate's float32 key is within ub - key of the real-number key
    L  (top-k passes) every eligible row outside the candidates has a real-number key >= thr_min
    C  (collect passes) every hit's key is <= the threshold; every eligible row whose real-number key is <= threshold -
       eps is among the hits -- every eligible row where the threshold is the "take everything" one (3e38)
    S  (sketch passes that settled) every eligible row outside the candidates is at reference distance >= D - slack

With the state of the sketch index (ScanIndex.sketch_info / sketch_rows) check() also asserts K_s, L_s and D -- K and L
for the sketch sweep's own keys, against the real-number keys of the sketch rows, and that D follows from thr_min --
and check_sketch_build() asserts B: the sketch bytes, the exception list and max_ang against sketch_reference().

Radius searches through the sketch (option sketch_radius, pass SZG_CERT_SKETCH_RADIUS) need no answer-dependent
certificate, only completeness; with the sketch state check() asserts K_s on their keyed entries and

    C_s  every eligible row in range that is no exception and whose real-number SKETCH key plus its rounding is <= thr -
         eps is among the keyed entries; every keyed entry has key <= thr; no ineligible row is collected
    T    thr - eps is at or above the real-number key the record's sketch-distance radius D implies: -cos(pi D)
         (cosine), (255 D / gscale)^2 (Euclid), in LD
    S_r  D >= radius + slack for the radius the test passed, and every eligible row with distance <= radius is among
         the record's entries or is an exception row

Top-k searches of large k through the sketch (option sketch_topk_collect, pass SZG_CERT_SKETCH_TOPK_COLLECT) find their
radius from a sample and then run that radius search: with the sketch state and the oracle's distances check() asserts
K_s, C_s and T as above on every record that carries a sweep (thr finite; an entry without a key is an exception row or
one of the query's first k eligible rows) and

    P    at least k eligible sketched rows have a real-number sketch key <= kmax (U), in LD where the case is small
    R    thr_min (tau) >= the sketch distance kmax implies -- acos(clamp(-kmax)) / pi (cosine), gscale sqrt(max(kmax, 0))
         / 255 (Euclid), in LD -- plus slack
    S_k  D >= thr_min (1 + 1e-9) + slack, and every eligible row at reference distance <= thr_min is among the
         record's entries or is an exception row
    F    a certified record's k-th oracle distance over the eligible rows is <= thr_min

Candidates the kernels force in carry no bound and are skipped and counted: cosine keys <= -1.5, rows with a non-finite
element or an overflowing norm, keys clamped to 3e38.  A zero cosine query claims no bound at all.
"""
import collections

import numpy as np

from . import _lib

PASS_NAMES = {_lib.SZG_CERT_TOPK: "topk", _lib.SZG_CERT_SKETCH: "sketch", _lib.SZG_CERT_ESCALATION: "escalation",
              _lib.SZG_CERT_RADIUS_SINGLE: "radius", _lib.SZG_CERT_RADIUS_SHARED: "radius-shared",
              _lib.SZG_CERT_SKETCH_RADIUS: "sketch-radius", _lib.SZG_CERT_SKETCH_TOPK_COLLECT: "sketch-topk-collect"}
# their keys are keys of the rows' sketches
SKETCH_PASSES = (_lib.SZG_CERT_SKETCH, _lib.SZG_CERT_SKETCH_RADIUS, _lib.SZG_CERT_SKETCH_TOPK_COLLECT)
COLLECT_SKETCH_PASSES = (_lib.SZG_CERT_SKETCH_RADIUS, _lib.SZG_CERT_SKETCH_TOPK_COLLECT)   # ... collected under a threshold
KEYS_NAMES = {-1: "-", _lib.SZG_CERT_KEYS_SINGLE: "Single", _lib.SZG_CERT_KEYS_SHARED_INT8: "SharedInt8",
              _lib.SZG_CERT_KEYS_SHARED_BF16: "SharedBf16", _lib.SZG_CERT_KEYS_BF16_BAND: "Bf16Band",
              _lib.SZG_CERT_KEYS_BF16_RESCORED: "Bf16Rescored"}
SWEEP_NAMES = {0: "one-sweep", 1: "int8", 2: "bf16"}
TAKE_ALL = float(np.float32(3.0e38))   # the threshold of a collect sweep that takes every row (and the clamp of a key)
LD = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
PI = 4 * np.arctan(LD(1))
WIDE_LIMIT = 2 * 10 ** 7  # (query, row, element) triples up to which the reference is computed in LD, element by element


def decode_rows(rows, dim, bits):
    """Packed rows -> float64[n, dim], the reference's decodeVector (big-endian fields; v / maxInt * 2 - 1)."""
    rb = {4: (dim + 1) // 2, 8: dim, 16: 2 * dim, 32: 4 * dim, 64: 8 * dim}[bits]
    r = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, rb)
    if bits == 64:
        return r.view(">f8").astype(np.float64)
    if bits == 32:
        return r.view(">f4").astype(np.float64)
    if bits == 16:
        v = r.view(">u2").astype(np.float64)
    elif bits == 8:
        v = r.astype(np.float64)
    else:
        v = np.empty((r.shape[0], 2 * rb), dtype=np.float64)
        v[:, 0::2] = r >> 4
        v[:, 1::2] = r & 15
        v = v[:, :dim]
    return v / float((1 << bits) - 1) * 2 - 1


class Corpus:
    """The packed rows of one collection and their real-number keys.  Rows are decoded and scored in slices, so a deep
    corpus never exists as one float64 matrix; X (every decoded row) is built only when asked for."""
    SLICE = 8192

    def __init__(self, rows, dim, bits, metric):
        self.dim, self.bits, self.metric = int(dim), int(bits), int(metric)
        rb = {4: (self.dim + 1) // 2, 8: self.dim, 16: 2 * self.dim, 32: 4 * self.dim, 64: 8 * self.dim}[self.bits]
        self.packed = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, rb)
        self.n = self.packed.shape[0]
        self.scale = float((1 << bits) - 1) if bits <= 16 else 1.0   # Euclidean keys are in units of 1 / maxInt
        self.finite = np.ones(self.n, dtype=bool)
        if bits >= 32:
            for lo in range(0, self.n, self.SLICE):
                self.finite[lo:lo + self.SLICE] = np.isfinite(self.rows(lo, lo + self.SLICE)).all(axis=1)
        self._kept = {}
        self._X = None

    def rows(self, lo, hi):
        return decode_rows(self.packed[lo:hi], self.dim, self.bits)

    @property
    def X(self):
        if self._X is None:
            self._X = self.rows(0, self.n)
        return self._X

    def with_metric(self, metric):
        """The same rows under the other metric (the packed rows are shared)."""
        return self if metric == self.metric else Corpus(self.packed, self.dim, self.bits, metric)

    def check_decode(self, orc, at=None):
        """Rows of the numpy decode against the oracle's decoder, bit for bit."""
        for r in (at if at is not None else sorted({0, self.n // 3, self.n - 1})):
            want = orc.decode_vector(self.packed[r], self.dim, self.bits)
            got = self.rows(r, r + 1)[0]
            assert ((got == want) | (np.isnan(got) & np.isnan(want))).all(), ("decode differs from the oracle's", r)

    def keys(self, Q):
        """-> (real[nq, n] float64, err[nq, n] float64): the real-number keys and a bound on their own rounding error."""
        Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
        tag = Q.tobytes()
        if tag in self._kept:
            return self._kept[tag]
        nq = Q.shape[0]
        wide = nq * self.n * self.dim <= WIDE_LIMIT
        dt = LD if wide else np.float64
        u = float(np.finfo(dt).eps)
        real = np.empty((nq, self.n), dtype=np.float64)
        err = np.empty_like(real)
        Qd = Q.astype(dt)
        qn2 = (Qd * Qd).sum(axis=1)
        with np.errstate(all="ignore"):
            for lo in range(0, self.n, self.SLICE):
                X = self.rows(lo, lo + self.SLICE).astype(dt)
                sl = slice(lo, lo + X.shape[0])
                xn2 = (X * X).sum(axis=1)
                if self.metric == _lib.SZG_COSINE:
                    dot = np.stack([(X * q).sum(axis=1) for q in Qd]) if wide else Qd @ X.T
                    real[:, sl] = (-dot / np.sqrt(qn2[:, None] * xn2[None, :])).astype(np.float64)
                    err[:, sl] = (self.dim + 8) * u   # |dot| <= |q||x|: the quotient is off by at most (dim + 8) u
                elif wide:
                    k = np.stack([((X - q) ** 2).sum(axis=1) for q in Qd]) * dt(self.scale) ** 2
                    real[:, sl] = k.astype(np.float64)
                    err[:, sl] = ((self.dim + 8) * u * k).astype(np.float64)
                else:   # the expanded form through one matrix product: its terms are bounded by (|x| + |q|)^2
                    real[:, sl] = (xn2[None, :] + qn2[:, None] - 2 * (Qd @ X.T)) * self.scale ** 2
                    err[:, sl] = 4 * (self.dim + 8) * u * (np.sqrt(xn2)[None, :] + np.sqrt(qn2)[:, None]) ** 2 * self.scale ** 2
        self._kept = {tag: (real, err)}
        return real, err


class Margins:
    """The largest |key - real| / (ub - key) seen per (pass, keys, sweep, row width, metric)."""

    def __init__(self):
        self.worst = collections.OrderedDict()
        self.count = collections.Counter()

    def note(self, what, ratio, n):
        self.worst[what] = max(self.worst.get(what, 0.0), float(ratio))
        self.count[what] += int(n)

    def lines(self):
        out = ["%-14s %-13s %-9s %5s %-6s %12s %10s" % ("pass", "keys", "sweep", "bits", "metric", "keys checked", "max ratio")]
        for (p, k, s, bits, metric), r in sorted(self.worst.items()):
            out.append("%-14s %-13s %-9s %5d %-6s %12d %10.4f" % (p, k, s, bits, "cosine" if metric else "euclid",
                                                                 self.count[(p, k, s, bits, metric)], r))
        return out


Summary = collections.namedtuple("Summary", "records kinds skipped skipped_rows checked")


def check(corpus, Q, recs, ents, dropped, eligible=None, dists=None, margins=None, what=(), sketch=None, radii=None):
    """Assert K, L, C and S for the records of ONE call with queries Q.  eligible: bool[n] or bool[nq, n] (None: every
    row); dists: float64[nq, n], the oracle's distances (needed for sketch records).  -> Summary; skipped_rows are the
    rows whose candidates carried no bound.

    sketch = (Corpus of the handle's sketch bytes at 8 bits, gscale, exc_rows) -- ScanIndex.sketch_rows / sketch_info
    after the call -- adds, for every sketch record with a finite thr_min (lb):

        K_s  each keyed entry's float32 sketch key is within ub - key of the real-number key of the row's SKETCH for
             the query the sweep saw (q / gscale under Euclid, q under cosine)
        L_s  every eligible row in range that is no exception and not among the keyed entries has a real-number
             sketch key >= thr_min
        D    the record's D is at most the sketch distance thr_min implies: acos(min(1, -thr_min)) / pi (cosine),
             gscale sqrt(max(thr_min, 0)) / 255 (Euclid), in LD, plus that expression's own rounding

    and, for every sketch-radius record (which needs sketch=, dists= and radii=, the radius the test passed per query):
    K_s, C_s, T and S_r as the module's docstring states them; for every sketch-topk-collect record (sketch= and dists=):
    P and R where kmax is finite, K_s, C_s, T and S_k where the record carries a sweep, F where it is certified."""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    nq, n = Q.shape[0], corpus.n
    assert dropped == 0, ("the trace dropped records", dropped, what)
    real, err = corpus.keys(Q)
    if sketch is not None:
        sk_corpus, gscale, exc_rows = sketch
        assert sk_corpus.bits == 8 and sk_corpus.n == n and sk_corpus.metric == corpus.metric, "the sketch corpus does not fit"
        euclid_s = corpus.metric != _lib.SZG_COSINE
        assert (gscale > 0) == euclid_s, ("gscale is positive exactly for Euclidean collections", gscale)
        real_s, err_s = sk_corpus.keys(Q / gscale if euclid_s else Q)
        is_exc = np.zeros(n, dtype=bool)
        is_exc[np.asarray(exc_rows, dtype=np.int64)] = True
    if eligible is None:
        eligible = np.ones(n, dtype=bool)
    eligible = np.broadcast_to(np.asarray(eligible, dtype=bool), (nq, n))
    zero_q = (Q == 0).all(axis=1) & (corpus.metric == _lib.SZG_COSINE)
    kinds = collections.Counter()
    skipped, checked, skipped_rows = 0, 0, set()
    for rec in recs:
        qi, p = int(rec["query"]), int(rec["pass_"])
        assert 0 <= qi < nq, ("query index out of the call", qi, what)
        e = ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]
        kind = (PASS_NAMES[p], KEYS_NAMES[int(rec["keys"])], SWEEP_NAMES[int(rec["sweep"])])
        kinds[kind] += 1
        where = what + (kind, "query", qi)
        rows = e["row"].astype(np.int64)
        assert ((rows >= 0) & (rows < n)).all(), ("row out of range", where)
        lo, hi = int(rec["row_lo"]), int(rec["row_hi"])
        in_range = np.zeros(n, dtype=bool)
        in_range[lo:hi] = True
        keyed = (e["flags"] & _lib.SZG_CERT_ENTRY_NO_KEY) == 0
        key = e["key"].astype(np.float64)
        ub = e["ub"]
        # ---- K
        if p not in SKETCH_PASSES and not zero_q[qi]:   # (a sketch key is the key of the row's 8-bit sketch, not of the row)
            r_real, r_err = real[qi, rows], err[qi, rows]
            forced = keyed & ((~corpus.finite[rows]) | ~np.isfinite(r_real) | (key >= TAKE_ALL) |
                              ((key <= -1.5) if corpus.metric == _lib.SZG_COSINE else False))
            skipped += int(forced.sum())
            skipped_rows.update(int(x) for x in rows[forced])
            ok = keyed & ~forced
            eps = ub[ok] - key[ok]
            assert (eps > 0).all(), ("a candidate without a bound", where)
            off = np.abs(key[ok] - r_real[ok])
            bad = off > eps + r_err[ok]
            assert not bad.any(), ("K: key outside its bound", where, "rows", rows[ok][bad][:8], "key", key[ok][bad][:8],
                                   "real", r_real[ok][bad][:8], "eps", eps[bad][:8], "of", int(ok.sum()))
            checked += int(ok.sum())
            if margins is not None and ok.any():
                margins.note(kind + (corpus.bits, corpus.metric), float((off / eps).max()), int(ok.sum()))
        outside = eligible[qi] & in_range
        outside[rows] = False
        outside &= np.isfinite(real[qi])   # (a row without a real-number key: NaN distance, never a neighbour)
        # ---- L
        if p == _lib.SZG_CERT_TOPK and np.isfinite(rec["thr_min"]) and not zero_q[qi]:
            low = real[qi] + err[qi] < rec["thr_min"]
            bad = np.flatnonzero(outside & low)
            assert bad.size == 0, ("L: a left-out row under the bound", where, "thr_min", float(rec["thr_min"]), "rows", bad[:8],
                                   "real", real[qi, bad[:8]])
        # ---- C
        if p in (_lib.SZG_CERT_ESCALATION, _lib.SZG_CERT_RADIUS_SINGLE, _lib.SZG_CERT_RADIUS_SHARED):
            thr = float(rec["thr"])
            assert (key <= thr).all(), ("C: a hit above the threshold", where, thr, key[key > thr][:8])
            if thr >= TAKE_ALL:
                missed = np.flatnonzero(eligible[qi] & in_range & ~np.isin(np.arange(n), rows))
            elif zero_q[qi]:
                missed = np.zeros(0, dtype=np.int64)
            else:
                assert np.isfinite(rec["eps"]) and rec["eps"] > 0, ("collect record without its bound", where)
                missed = np.flatnonzero(outside & (real[qi] + err[qi] <= thr - rec["eps"]))
            assert missed.size == 0, ("C: an eligible row under the threshold was not collected", where, "thr", thr, "eps",
                                      float(rec["eps"]), "rows", missed[:8], "real", real[qi, missed[:8]])
            inel = ~eligible[qi, rows]
            assert not inel.any(), ("C: a row that is not eligible was collected", where, rows[inel][:8])
        # ---- K_s, L_s, D
        if p == _lib.SZG_CERT_SKETCH_RADIUS:
            assert sketch is not None and dists is not None and radii is not None, \
                "sketch-radius records need the sketch state, the oracle's distances and the radii"
            assert not zero_q[qi], ("a zero cosine query is handed over, never recorded", where)
        topk_c = p == _lib.SZG_CERT_SKETCH_TOPK_COLLECT
        if topk_c:
            assert sketch is not None and dists is not None, \
                "sketch-topk-collect records need the sketch state and the oracle's distances"
            k = int(rec["k"])
            assert k >= 1 and rec["certified"] in (0, 1), ("a sketch-topk-collect record without k or its verdict", where)
            if zero_q[qi]:
                assert rec["certified"] == 0 and len(e) == 0, ("a zero cosine query is handed over", where)
            elig_s = eligible[qi] & in_range & ~is_exc & np.isfinite(real_s[qi])
            if np.isfinite(rec["kmax"]) and not zero_q[qi]:
                kmax, tau = float(rec["kmax"]), float(rec["thr_min"])
                # ---- P
                under = int((elig_s & (real_s[qi] - err_s[qi] <= kmax)).sum())
                assert under >= k, ("P: fewer than k eligible sketched rows with a real-number sketch key <= kmax", where,
                                    "kmax", kmax, "rows under it", under, "k", k)
                # ---- R
                if euclid_s:
                    implied = LD(gscale) * np.sqrt(LD(max(kmax, 0.0))) / LD(255)
                else:
                    implied = np.arccos(LD(max(-1.0, min(1.0, -kmax)))) / PI
                implied = float(implied)
                assert tau >= implied + float(rec["slack"]) - 4 * np.finfo(np.float64).eps * (implied + float(rec["slack"])), (
                    "R: thr_min below the distance kmax implies plus slack", where, tau, implied, float(rec["slack"]), kmax)
            # ---- F
            if rec["certified"] == 1:
                assert np.isfinite(rec["thr"]) and np.isfinite(rec["kmax"]), ("a certified record without its sweep", where)
                d_el = dists[qi][eligible[qi] & in_range]
                d_el = np.sort(d_el[~np.isnan(d_el)])
                assert d_el.size >= k and d_el[k - 1] <= rec["thr_min"], (
                    "F: the k-th oracle distance is above thr_min", where, float(rec["thr_min"]),
                    float(d_el[k - 1]) if d_el.size >= k else None)
        if p in SKETCH_PASSES and sketch is not None and not zero_q[qi] and \
                (p == _lib.SZG_CERT_SKETCH_RADIUS or (topk_c and np.isfinite(rec["thr"])) or
                 (p == _lib.SZG_CERT_SKETCH and np.isfinite(rec["thr_min"]))):
            lb = float(rec["thr_min"])
            s_real, s_err = real_s[qi, rows], err_s[qi, rows]
            forced = keyed & (~np.isfinite(s_real) | (key >= TAKE_ALL) | ((key <= -1.5) if not euclid_s else False))
            skipped += int(forced.sum())
            skipped_rows.update(int(x) for x in rows[forced])
            ok = keyed & ~forced
            eps = ub[ok] - key[ok]
            assert (eps > 0).all(), ("K_s: a sketch candidate without a bound", where)
            off = np.abs(key[ok] - s_real[ok])
            bad = off > eps + s_err[ok]
            assert not bad.any(), ("K_s: sketch key outside its bound", where, "rows", rows[ok][bad][:8], "key", key[ok][bad][:8],
                                   "real", s_real[ok][bad][:8], "eps", eps[bad][:8], "of", int(ok.sum()))
            checked += int(ok.sum())
            if margins is not None and ok.any():
                margins.note(("sketch K_s", kind[1], kind[2], 8, corpus.metric), float((off / eps).max()), int(ok.sum()))
            left = eligible[qi] & in_range & ~is_exc & np.isfinite(real_s[qi])
            left[rows[keyed]] = False
            if p in COLLECT_SKETCH_PASSES:
                # ---- C_s
                thr, r_eps = float(rec["thr"]), float(rec["eps"])
                assert (key[keyed] <= thr).all(), ("C_s: a collected sketch key above the threshold", where, thr,
                                                   key[keyed][key[keyed] > thr][:8])
                assert np.isfinite(r_eps) and r_eps > 0, ("C_s: the record carries no bound", where)
                if thr >= TAKE_ALL:
                    missed = np.flatnonzero(left)
                else:
                    missed = np.flatnonzero(left & (real_s[qi] + err_s[qi] <= thr - r_eps))
                assert missed.size == 0, ("C_s: an eligible sketched row under the threshold was not collected", where, "thr",
                                          thr, "eps", r_eps, "rows", missed[:8], "real", real_s[qi, missed[:8]])
                inel = ~eligible[qi, rows]
                assert not inel.any(), ("C_s: a row that is not eligible was collected", where, rows[inel][:8])
                assert not is_exc[rows[keyed]].any(), ("C_s: a row without a usable sketch among the keyed entries", where)
                beside = is_exc[rows[~keyed]]
                if topk_c:   # (the query's first k eligible rows are staged beside the exception rows)
                    first_k = np.zeros(n, dtype=bool)
                    first_k[np.flatnonzero(eligible[qi])[:k]] = True
                    beside = beside | first_k[rows[~keyed]]
                assert beside.all(), ("C_s: an entry without a key that is no exception row", where)
                # ---- T
                D = LD(float(rec["D"]))
                assert np.isfinite(float(D)) and (euclid_s or float(D) < 1.0), ("T: a radius that is handed over was recorded", where)
                implied = float((LD(255) * D / LD(gscale)) ** 2 if euclid_s else -np.cos(PI * D))
                assert thr - r_eps >= implied - 4 * np.finfo(np.float64).eps * abs(implied), (
                    "T: thr - eps below the key the sketch-distance radius implies", where, thr, r_eps, implied, float(D))
                if topk_c:
                    # ---- S_k
                    tau = float(rec["thr_min"])
                    assert rec["D"] >= tau * (1.0 + 1e-9) + rec["slack"], ("S_k: the sketch-distance radius does not cover "
                                                                         "thr_min (1 + 1e-9) + slack", where, float(rec["D"]),
                                                                         tau, float(rec["slack"]))
                    d = dists[qi]
                    hit = eligible[qi] & in_range & (d <= tau)
                    hit[rows] = False
                    bad = np.flatnonzero(hit & ~is_exc)
                    assert bad.size == 0, ("S_k: a row within thr_min is neither an entry nor an exception row", where, tau,
                                           "rows", bad[:8], "dist", d[bad[:8]])
                    continue
                # ---- S_r
                radius = float(np.broadcast_to(np.asarray(radii, dtype=np.float64), (nq,))[qi])
                assert rec["D"] >= radius + rec["slack"], ("S_r: the sketch-distance radius does not cover radius + slack", where,
                                                          float(rec["D"]), radius, float(rec["slack"]))
                d = dists[qi]
                hit = eligible[qi] & in_range & (d <= radius)
                hit[rows] = False
                bad = np.flatnonzero(hit & ~is_exc)
                assert bad.size == 0, ("S_r: a row within the radius is neither an entry nor an exception row", where, radius,
                                       "rows", bad[:8], "dist", d[bad[:8]])
                continue
            bad = np.flatnonzero(left & (real_s[qi] + err_s[qi] < lb))
            assert bad.size == 0, ("L_s: a sketched row outside the lists under the bound", where, "thr_min", lb, "rows", bad[:8],
                                   "real", real_s[qi, bad[:8]])
            if np.isfinite(rec["D"]):
                if euclid_s:
                    implied = LD(gscale) * np.sqrt(LD(max(lb, 0.0))) / LD(255)
                else:
                    implied = np.arccos(LD(max(-1.0, min(1.0, -lb)))) / PI
                implied = float(implied)
                assert rec["D"] <= implied + 4 * np.finfo(np.float64).eps * implied, ("D: above the distance thr_min implies",
                                                                                      where, float(rec["D"]), implied, lb)
        # ---- S
        if p == _lib.SZG_CERT_SKETCH and rec["certified"] == 1 and np.isfinite(rec["D"]):
            assert dists is not None, "sketch records need the oracle's distances"
            d = dists[qi]
            bad = np.flatnonzero(outside & (d < rec["D"] - rec["slack"]))
            assert bad.size == 0, ("S: a row outside the candidates nearer than D - slack", where, float(rec["D"]),
                                   float(rec["slack"]), "rows", bad[:8], "dist", d[bad[:8]])
    return Summary(len(recs), kinds, skipped, skipped_rows, checked)


# ---- the sketch index: bytes, exceptions and max_ang (B) ---------------------------------------------------------------

def sketch_angle_rounding(dim):
    """What sketch_slack (sketch_bound.h) adds to max_ang under cosine for the rounding of the build kernel's float64
    angles: the device's cosine of (row, sketch) is off by at most (dim + 8) u, which acos turns into at most
    sqrt(2 (dim + 8) u) near c = 1; twice the root covers a float64 reference beside it.  1e-7 up to dim 103."""
    return max(1e-7, 2.0 * np.sqrt((dim + 8) * 2.0 ** -52) / np.pi)


def sketch_slack(max_ang, gscale, dim):
    """slack as sketch_slack (sketch_bound.h) forms it from the sketch state; tests/test_sketch_bound_cpu.py holds the two
    to equal bits."""
    return max_ang * (1.0 + 1e-9) + (0.0 if gscale > 0 else sketch_angle_rounding(dim))


def sketch_reference(vec, metric, gscale):
    """What sketch_build_kernel -- and sketch_build_f64_kernel, for float64 rows under option sketch_f64 -- is specified to
    do with rows vec[n, dim] (the rows' values as float64: decode_rows(..., 32) or decode_rows(..., 64)) ->
    (t[n, dim] in LD, must_exc[n]): the ideal scaled value t = (x / scale + 1) * 127.5, whose nearest integer clipped to
    0..255 is the row's sketch byte -- scale is the row's largest |x_i| under cosine and gscale under Euclid -- and
    whether the row has no usable sketch: a non-finite element, no direction (all zero, cosine), an element beyond
    gscale (Euclid).  t of such a row means nothing."""
    X = np.asarray(vec, dtype=np.float64)
    fin = np.isfinite(X)
    finite = fin.all(axis=1)
    mx = np.abs(np.where(fin, X, 0.0)).max(axis=1)
    if metric == _lib.SZG_COSINE:
        must = ~finite | (mx == 0)
        scale = mx
    else:
        must = ~finite | (mx > gscale)
        scale = np.full(X.shape[0], float(gscale))
    scale = np.where(must, 1.0, scale)
    with np.errstate(all="ignore"):
        t = (X.astype(LD) / scale.astype(LD)[:, None] + LD(1)) * LD(127.5)
    return t, must


def check_sketch_build(vec, sk_bytes, info, exc_rows, rebuilt, metric=None, rec_slack=None, what=()):
    """Assert B for the sketch state (info: ScanIndex.sketch_info(); sk_bytes: uint8[n, dim], ScanIndex.sketch_rows())
    of float32 or float64 rows with values vec[n, dim]; rebuilt: the last sync built every row anew.  The reference is
    computed in LD, whose exponent range (x87: 15 bits) holds the squares of any double: rows at 1e-150 or 1e200 are
    checked like any other.

        B1  every byte of a sketched row is within 0.5 + 1e-9 of clip(t, 0, 255) (the device may fuse the multiply-add:
            a tie may fall either way); every byte of a row that must be an exception is 128
        B2  every row that must be an exception is listed; after a rebuild nothing else is
        B3  d(row, decoded sketch) <= slack for every sketched row, in LD: acos(c) / pi against
            max_ang (1 + 1e-9) + sketch_angle_rounding(dim), or the norm of row - gscale n / 255 against
            max_ang (1 + 1e-9); rec_slack, a traced record's, agrees with that slack
        B4  max_ang >= the largest such distance less the reference's rounding -- and, rebuilt, <= it plus the rounding.
            The rounding: both cosines are off by at most (dim + 8) u, acos amplifies by 1 / sqrt(1 - c^2), capped at
            sqrt(2 (dim + 8) u); it must stay below what the search adds for it.  Euclid: (dim + 8) u relative.
        scale (Euclid)  gscale is the largest |x_i| of the rows without a non-finite element, exactly (1 where there is
            none), after a rebuild; else at least that of the rows not listed as exceptions

    -> dict: sketched, exceptions, largest (the reference's), allowance, share (largest / slack)."""
    X = np.asarray(vec, dtype=np.float64)
    n, dim = X.shape
    gscale, max_ang = float(info["gscale"]), float(info["max_ang"])
    if metric is None:
        metric = _lib.SZG_COSINE if gscale == 0 else 1 - _lib.SZG_COSINE
    euclid = metric != _lib.SZG_COSINE
    assert (gscale > 0) == euclid, ("gscale is positive exactly for Euclidean collections", gscale, what)
    sk_bytes = np.asarray(sk_bytes)
    assert sk_bytes.dtype == np.uint8 and sk_bytes.shape == (n, dim), ("dim bytes per sketch row", sk_bytes.shape, (n, dim), what)
    assert int(info["rows"]) == n and int(info["n_exc"]) == len(exc_rows), (what, info)
    t, must = sketch_reference(X, metric, gscale)
    exc = np.zeros(n, dtype=bool)
    exc[np.asarray(exc_rows, dtype=np.int64)] = True
    # ---- B2
    missing = np.flatnonzero(must & ~exc)
    assert missing.size == 0, ("B2: a row without a usable sketch is not an exception", what, missing[:8])
    if rebuilt:
        more = np.flatnonzero(exc & ~must)
        assert more.size == 0, ("B2: an exception after a rebuild that need not be one", what, more[:8])
    # ---- B1
    bad = np.flatnonzero((sk_bytes[must] != 128).any(axis=1))
    assert bad.size == 0, ("B1: an exception row's bytes are not all 128", what, np.flatnonzero(must)[bad][:8])
    at = np.flatnonzero(~must)
    v = sk_bytes[at].astype(LD)
    off = np.abs(v - np.clip(t[at], 0, 255))
    bad = off > 0.5 + 1e-9
    assert not bad.any(), ("B1: a sketch byte is not the nearest", what, "rows", at[bad.any(axis=1)][:8], "bytes",
                           sk_bytes[at][bad][:8], "ideal", t[at][bad][:8].astype(np.float64))
    # ---- scale
    fin_rows = np.isfinite(X).all(axis=1)
    if euclid:
        if rebuilt:
            top = np.abs(X[fin_rows]).max() if fin_rows.any() else 0.0
            assert gscale == (top if top > 0 else 1.0), ("scale: not the largest finite |x_i|", what, gscale, top)
        else:
            have = fin_rows & ~exc
            top = np.abs(X[have]).max() if have.any() else 0.0
            assert gscale >= top, ("scale: below a sketched row's largest |x_i|", what, gscale, top)
    # ---- B3
    slack = sketch_slack(max_ang, gscale, dim)
    if rec_slack is not None:
        assert abs(float(rec_slack) - slack) <= 4 * np.finfo(np.float64).eps * slack, ("the search's slack is not the state's",
                                                                                       what, float(rec_slack), slack)
    u = float(np.finfo(np.float64).eps) + float(np.finfo(LD).eps)
    Xs, nvec = X[at].astype(LD), 2 * v - 255
    with np.errstate(all="ignore"):
        if euclid:
            d = np.sqrt(((Xs - LD(gscale) * nvec / 255) ** 2).sum(axis=1))
            allow = (dim + 8) * u * d
        else:
            c = (Xs * nvec).sum(axis=1) / np.sqrt((Xs * Xs).sum(axis=1) * (nvec * nvec).sum(axis=1))
            c = np.clip(c, -1, 1)
            d = np.arccos(c) / PI
            dc = (dim + 8) * u
            sin = np.sqrt(np.maximum(1 - c * c, 0))
            allow = np.minimum(dc / np.maximum(sin, LD(1e-300)), np.sqrt(2 * dc)) / PI + 4 * np.finfo(np.float64).eps
    d, allow = d.astype(np.float64), allow.astype(np.float64)
    assert np.isfinite(d).all(), ("the reference's own distance is not finite", what, at[~np.isfinite(d)][:8])
    bad = d > slack
    assert not bad.any(), ("B3: a row farther from its sketch than slack", what, "rows", at[bad][:8], "dist", d[bad][:8], "slack", slack)
    # ---- B4
    largest = float(d.max()) if d.size else 0.0
    allowance = float(allow.max()) if d.size else 0.0
    if not euclid:
        assert allowance < sketch_angle_rounding(dim), ("the angles' rounding is not below what the search adds for it", what,
                                                        allowance, sketch_angle_rounding(dim))
    assert max_ang >= largest - allowance, ("B4: max_ang below the largest row-to-sketch distance", what, max_ang, largest, allowance)
    if rebuilt:
        assert max_ang <= largest + allowance, ("B4: max_ang above the largest row-to-sketch distance after a rebuild", what,
                                                max_ang, largest, allowance)
    return {"sketched": int(at.size), "exceptions": int(exc.sum()), "largest": largest, "allowance": allowance,
            "share": largest / slack if slack > 0 else 0.0}


# ---- the bfloat16 sweeps, operand by operand ------------------------------------------------------------------------

def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even) as float32, by bit arithmetic (v_cvt_pk_bf16_f32; scan_query.cpp
    bf16_rne).  Finite values only."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _bf16_query(corpus, q):
    """One query as the sweeps stage it: (the bfloat16 image as float64, |g|^2 of the unrounded prepared query)."""
    m1 = 0.0
    for v in q:           # (in the order prep_query_norms sums it)
        m1 += float(v) * float(v)
    if corpus.metric == _lib.SZG_COSINE:
        scale = 1.0 / np.sqrt(m1) if m1 > 0 else 0.0
    else:
        scale = {16: 65535.0, 8: 255.0}.get(corpus.bits, 1.0)
    g = (q * scale).astype(np.float32)
    return bf16_round(g).astype(np.float64), float(((q * scale) ** 2).sum())


def bf16_emulated(corpus, Q, queries, rows=None):
    """The keys the bfloat16 sweeps would give rows `rows` (None: every row) for the listed queries if the matrix core
    summed exactly, and the float32-accumulation part of key_eps's bfloat16 branch at those keys (4 n u, cosine;
    3 n u s^2 + 4 n 2^-126, Euclid: the second term is float32's underflow, which the float64 emulation does not have): two arrays [len(queries), len(rows)].

    Operands, as build_image_bf16 and the kernels form them: the query is q / |q| (cosine) or maxInt * q (Euclid, rows
    of 16 or 8 bits; q itself otherwise), narrowed to float32 and rounded to bfloat16.  A row element is the float32
    value (32-bit rows), the float64 value narrowed to float32 (64-bit rows) or the code n = 2 v - maxInt (16- and
    8-bit rows, exact in float32); 32-, 64- and 16-bit elements are rounded to bfloat16, an 8-bit row's n enters
    exactly (the kernel multiplies v - 128, exact in bfloat16, and adds the sum of the rounded query).  The row's norm
    is the float32 sum of the squares of the UNROUNDED float32 elements -- summed in the sweep or read from the
    resident array, the same float either way -- and the Euclidean |g|^2 is that of the unrounded prepared query, so no
    term of the formula beyond the accumulation part is needed for them."""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    staged = [_bf16_query(corpus, Q[qi]) for qi in queries]
    GB = np.stack([g for g, _ in staged])
    qnorm2 = np.array([x for _, x in staged])
    rows = np.arange(corpus.n) if rows is None else np.asarray(rows, dtype=np.int64)
    dot = np.empty((len(staged), rows.size))
    nrm = np.empty(rows.size)
    for lo in range(0, rows.size, Corpus.SLICE):
        X = decode_rows(corpus.packed[rows[lo:lo + Corpus.SLICE]], corpus.dim, corpus.bits)
        if corpus.bits <= 16:
            x32 = np.rint((X + 1) / 2 * corpus.scale) * 2 - corpus.scale   # n = 2 v - maxInt
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                x32 = X.astype(np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            xb = x32 if corpus.bits == 8 else bf16_round(x32.astype(np.float32)).astype(np.float64)
            dot[:, lo:lo + X.shape[0]] = GB @ xb.T
            nrm[lo:lo + X.shape[0]] = (x32 * x32).sum(axis=1)
    u, nn = 2.0 ** -24, corpus.dim + 16.0 + (4.0 if corpus.bits == 64 else 0.0)
    with np.errstate(all="ignore"):
        if corpus.metric == _lib.SZG_COSINE:
            return -dot / np.sqrt(nrm)[None, :], np.full(dot.shape, 4.0 * nn * u)
        key = nrm[None, :] + qnorm2[:, None] - 2 * dot
        s = 2.0 * np.sqrt(qnorm2)[:, None] + np.sqrt(np.abs(key))
        # (the emulation sums in float64, whose range the sweep's float32 sums do not have: a term below the smallest
        # normal float32 may be lost whole, to underflow or to the matrix core's flush -- 2^-126 per term of the three
        # sums and the finish.  A query within a subnormal spacing of an all-zero row has an emulated key of 1e-90 and
        # a float32 key of 0; key_eps carries 1e-30 for the same reason.)
        return key, 3.0 * nn * u * s * s + 4.0 * nn * 2.0 ** -126


def check_bf16_tight(corpus, Q, recs, ents, margins=None, what=()):
    """Every keyed, unforced candidate of the records whose keys are the bfloat16 sweep's own -- SharedBf16 lists and
    collect records of a shared bfloat16 sweep -- lies within the accumulation part of the bound of the emulated key.
    -> keys checked."""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    own = [rec for rec in recs
           if ((rec["pass_"] == _lib.SZG_CERT_TOPK and rec["keys"] == _lib.SZG_CERT_KEYS_SHARED_BF16) or
               (rec["pass_"] == _lib.SZG_CERT_RADIUS_SHARED and rec["sweep"] == 2)) and
           not (corpus.metric == _lib.SZG_COSINE and not Q[int(rec["query"])].any())]
    if not own:
        return 0
    # many entries (an all-rows radius batch): every (query, row) pair at once; a few lists: their rows only
    whole = sum(int(rec["n_entries"]) for rec in own) >= corpus.n
    if whole:
        order = sorted({int(rec["query"]) for rec in own})
        at = {qi: i for i, qi in enumerate(order)}
        all_emul, all_tol = bf16_emulated(corpus, Q, order)
    checked = 0
    for rec in own:
        qi = int(rec["query"])
        e = ents[int(rec["first_entry"]): int(rec["first_entry"] + rec["n_entries"])]
        rows = e["row"].astype(np.int64)
        key = e["key"].astype(np.float64)
        if whole:
            emul, tol = all_emul[at[qi], rows], all_tol[at[qi], rows]
        else:
            emul, tol = (x[0] for x in bf16_emulated(corpus, Q, [qi], rows))
        ok = corpus.finite[rows] & np.isfinite(emul) & (key < TAKE_ALL)
        if corpus.metric == _lib.SZG_COSINE:
            ok &= key > -1.5
        off = np.abs(key - emul)
        bad = ok & (off > tol)
        assert not bad.any(), ("bfloat16 key outside the accumulation part of its bound", what, "query", qi, "rows",
                               rows[bad][:8], "key", key[bad][:8], "emulated", emul[bad][:8], "tolerance", tol[bad][:8])
        checked += int(ok.sum())
        if margins is not None and ok.any():
            margins.note(("bf16-operands", KEYS_NAMES[int(rec["keys"])], PASS_NAMES[int(rec["pass_"])], corpus.bits,
                          corpus.metric), float((off[ok] / tol[ok]).max()), int(ok.sum()))
    return checked
