"""The sketch checks of syzgydb_amd/cert_check.py on their own, without a device.

tests/test_gpu_sketch_state.py holds the card's sketch bytes, exception list, max_ang and sweep keys against
cert_check.sketch_reference / check_sketch_build / check(sketch=...).  Here the sketch is made with numpy as
sketch_build_kernel is specified (byte = clip(rint((x / scale + 1) * 127.5), 0, 255), 128 for a row without a usable
sketch, max_ang = the largest d(row, decoded sketch)) and a sketch sweep's record is made from float64 keys, so that

  * the triangle inequality the pre-pass rests on holds with the oracle's own distances,
  * the checks pass on a sketch that is right, and
  * each deliberate corruption -- a byte, max_ang, the exception list, a list entry -- makes them raise.
"""
import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import _lib
from syzgydb_amd import cert_check as cc

METRICS = (0, 1)   # Euclidean, cosine
DIM, N, KP, K = 40, 600, 40, 5


def numpy_sketch(X, metric):
    """float32 row values X[n, dim] -> (bytes, info, exc_rows) as a full rebuild would leave them."""
    fin = np.isfinite(X).all(axis=1)
    mx = np.abs(np.where(np.isfinite(X), X, 0.0)).max(axis=1)
    if metric == _lib.SZG_COSINE:
        gscale, bad = 0.0, ~fin | (mx == 0)
        scale = mx
    else:
        gscale = float(mx[fin].max()) if fin.any() and mx[fin].max() > 0 else 1.0
        bad = ~fin
        scale = np.full(X.shape[0], gscale)
    with np.errstate(all="ignore"):
        v = np.clip(np.rint((X * (1.0 / np.where(bad, 1.0, scale))[:, None] + 1.0) * 127.5), 0, 255)
    v[bad] = 128
    v = v.astype(np.uint8)
    nvec = 2.0 * v[~bad] - 255.0
    if gscale > 0:
        d = np.sqrt(((X[~bad] - gscale * nvec / 255.0) ** 2).sum(axis=1))
    else:
        c = (X[~bad] * nvec).sum(axis=1) / np.sqrt((X[~bad] ** 2).sum(axis=1) * (nvec ** 2).sum(axis=1))
        d = np.arccos(np.clip(c, -1, 1)) / np.pi
    exc = np.flatnonzero(bad).astype(np.uint64)
    info = {"exists": 1, "in_sync": 1, "disabled": 0, "rows": X.shape[0], "max_ang": float(d.max()), "gscale": gscale,
            "n_exc": exc.size}
    return v, info, exc


def rows_and_queries(metric):
    vec = orc.synth_vectors(0x5B00 + metric, 0, N, DIM)
    # (one shared scale under Euclid: a wide spread of row lengths leaves the short rows no bytes, and nothing settles)
    vec *= 10.0 ** np.linspace(-0.2, 0.2, N)[:, None] if metric == 0 else 10.0 ** np.linspace(-30, 30, N)[:, None]
    vec[3] = 0.0
    vec[4] = 0.0
    vec[4, 7] = -2.5                      # one non-zero element
    vec[5] = np.where(np.arange(DIM) % 3 == 0, -0.75, 0.75)   # every |x_i| equal: the sketch is exact under cosine
    vec[6, 0] = np.inf
    vec[7, DIM - 1] = np.nan
    packed = orc.encode_rows(vec, 32)
    X = cc.decode_rows(packed, DIM, 32)   # the float32 values
    near = X[[20, 300, 500]]
    if metric == _lib.SZG_COSINE:
        near = near / np.abs(near).max(axis=1)[:, None]
    Q = near + 0.01 * orc.synth_vectors(0x5B10 + metric, 0, 3, DIM)
    return packed, X, Q


def sketch_records(corpus, sk_corpus, info, exc, Q, dists):
    """One sketch record per query as SketchCall::settle writes it, its list the KP best float64 sketch keys narrowed
    to float32, with a bound of 1e-5 |key| + 1e-6 per key."""
    euclid = corpus.metric != _lib.SZG_COSINE
    gs = info["gscale"]
    real_s, _ = sk_corpus.keys(Q / gs if euclid else Q)
    slack = cc.sketch_slack(info["max_ang"], gs, corpus.dim)
    recs = np.zeros(Q.shape[0], dtype=np.dtype(_lib.SzgCertRecord))
    ents = []
    for qi in range(Q.shape[0]):
        order = np.argsort(real_s[qi], kind="stable")[:KP]
        key = real_s[qi, order].astype(np.float32)
        eps = np.abs(key.astype(np.float64)) * 1e-5 + 1e-6
        lb = float(key[-1]) - eps[-1]
        if euclid:
            D = gs * np.sqrt(max(lb, 0.0)) / 255.0 * (1.0 - 1e-9)
        else:
            x = -lb + 1e-15
            D = 0.0 if x >= 1 else np.arccos(x) / np.pi * (1.0 - 1e-12)
        first = len(ents)
        for r, kf, e in zip(order, key, eps):
            ents.append((int(r), dists[qi, r], float(kf) + e, kf, 0))
        for r in exc:
            ents.append((int(r), dists[qi, int(r)], 0.0, 0.0, _lib.SZG_CERT_ENTRY_NO_KEY))
        cand = np.concatenate([order, exc.astype(np.int64)])
        dk = np.sort(dists[qi, cand][np.isfinite(dists[qi, cand])])[K - 1]
        rec = recs[qi]
        rec["query"], rec["pass_"], rec["keys"], rec["sweep"], rec["k"] = qi, _lib.SZG_CERT_SKETCH, _lib.SZG_CERT_KEYS_SINGLE, 0, K
        rec["certified"] = int(dk * (1.0 + 1e-9) < D - slack)
        rec["row_lo"], rec["row_hi"] = 0, corpus.n
        rec["thr_min"], rec["D"], rec["slack"] = lb, D, slack
        rec["kmax"] = rec["thr"] = rec["eps"] = np.nan
        rec["first_entry"], rec["n_entries"] = first, len(ents) - first
    return recs, np.array(ents, dtype=np.dtype(_lib.SzgCertEntry))


@pytest.mark.parametrize("metric", METRICS, ids=["euc", "cos"])
def test_triangle_inequality_with_the_oracles_distances(metric):
    """|d(q, x) - d(q, sketch of x)| <= max d(x, sketch) + 1e-7, every distance the oracle's: the 8-bit rows decode to
    n / 255, the sketch's direction under cosine and the sketch over gscale under Euclid."""
    packed, X, Q = rows_and_queries(metric)
    v, info, exc = numpy_sketch(X, metric)
    got = cc.check_sketch_build(X, v, info, exc, True, metric=metric)
    assert got["sketched"] == N - exc.size and got["share"] <= 1.0
    keep = np.ones(N, dtype=bool)
    keep[exc.astype(np.int64)] = False
    for q in Q:
        d_row = orc.all_distances(packed, DIM, 32, metric, q)
        if metric == _lib.SZG_COSINE:
            d_sk = orc.all_distances(v, DIM, 8, metric, q)
        else:
            d_sk = info["gscale"] * orc.all_distances(v, DIM, 8, metric, q / info["gscale"])
        gap = np.abs(d_row[keep] - d_sk[keep])
        assert (gap <= got["largest"] + 1e-7).all(), (metric, float(gap.max()), got["largest"])


@pytest.mark.parametrize("metric", METRICS, ids=["euc", "cos"])
def test_build_check_raises_on_each_corruption(metric):
    packed, X, Q = rows_and_queries(metric)
    v, info, exc = numpy_sketch(X, metric)
    slack = cc.sketch_slack(info["max_ang"], info["gscale"], DIM)
    cc.check_sketch_build(X, v, info, exc, True, metric=metric, rec_slack=slack)
    assert (set(int(r) for r in exc) == {6, 7}) if metric == 0 else (set(int(r) for r in exc) == {3, 6, 7})
    # a byte two steps off
    bad = v.copy()
    bad[100, 11] = bad[100, 11] + 2 if bad[100, 11] < 200 else bad[100, 11] - 2
    with pytest.raises(AssertionError, match="B1"):
        cc.check_sketch_build(X, bad, info, exc, True, metric=metric)
    # an exception row that kept real bytes
    bad = v.copy()
    bad[6, 5] = 127
    with pytest.raises(AssertionError, match="B1"):
        cc.check_sketch_build(X, bad, info, exc, True, metric=metric)
    # max_ang shrunk: some row is farther from its sketch than slack (B3), and a stale-high one fails only a rebuild
    with pytest.raises(AssertionError, match="B3"):
        cc.check_sketch_build(X, v, dict(info, max_ang=info["max_ang"] * 0.5), exc, False, metric=metric)
    cc.check_sketch_build(X, v, dict(info, max_ang=info["max_ang"] * 1.5), exc, False, metric=metric)
    with pytest.raises(AssertionError, match="B4"):
        cc.check_sketch_build(X, v, dict(info, max_ang=info["max_ang"] * 1.5), exc, True, metric=metric)
    # a row that must be an exception is not listed; a listed one that need not be, after a rebuild
    with pytest.raises(AssertionError, match="B2"):
        cc.check_sketch_build(X, v, dict(info, n_exc=exc.size - 1), exc[:-1], True, metric=metric)
    more = np.sort(np.append(exc, np.uint64(50)))
    cc.check_sketch_build(X, v, dict(info, n_exc=more.size), more, False, metric=metric)
    with pytest.raises(AssertionError, match="B2"):
        cc.check_sketch_build(X, v, dict(info, n_exc=more.size), more, True, metric=metric)
    # the search's slack is not the state's
    with pytest.raises(AssertionError, match="slack"):
        cc.check_sketch_build(X, v, info, exc, True, metric=metric, rec_slack=slack * (1 + 1e-6))
    if metric == 0:   # (bytes made for one scale do not fit another: B1 speaks before the scale's own check)
        with pytest.raises(AssertionError, match="B1|scale"):
            cc.check_sketch_build(X, v, dict(info, gscale=info["gscale"] * 2), exc, True, metric=metric)


@pytest.mark.parametrize("metric", METRICS, ids=["euc", "cos"])
def test_key_and_list_checks_raise_on_each_corruption(metric):
    packed, X, Q = rows_and_queries(metric)
    v, info, exc = numpy_sketch(X, metric)
    corpus = cc.Corpus(packed, DIM, 32, metric)
    sk_corpus = cc.Corpus(v, DIM, 8, metric)
    dists = np.stack([orc.all_distances(packed, DIM, 32, metric, q) for q in Q])
    recs, ents = sketch_records(corpus, sk_corpus, info, exc, Q, dists)
    sketch = (sk_corpus, info["gscale"], exc)
    margins = cc.Margins()
    s = cc.check(corpus, Q, recs, ents, 0, dists=dists, margins=margins, sketch=sketch)
    assert s.checked == Q.shape[0] * KP and s.skipped == 0
    assert (recs["certified"] == 1).any(), "no record settled: S did not run"
    assert [w[0] for w in margins.worst] == ["sketch K_s"] and max(margins.worst.values()) <= 1.0
    # without the sketch state nothing of it is checked (the records alone pass S)
    assert cc.check(corpus, Q, recs, ents, 0, dists=dists).checked == 0
    # L_s: the first entry of the first list is removed -- a sketched row under the bound is now outside the lists
    rec = recs[0]
    assert ents["key"][0] + 1e-3 * abs(ents["key"][0]) < rec["thr_min"] and int(ents["row"][0]) not in set(int(r) for r in exc)
    fewer = np.delete(ents, 0)
    r2 = recs.copy()
    r2["n_entries"][0] -= 1
    r2["first_entry"][1:] -= 1
    with pytest.raises(AssertionError, match="L_s"):
        cc.check(corpus, Q, r2, fewer, 0, dists=dists, sketch=sketch)
    # K_s: a key beyond its bound
    e2 = ents.copy()
    e2["key"][1] = e2["key"][1] + 10 * (e2["ub"][1] - e2["key"][1]) + np.float32(1e-3) * abs(e2["key"][1])
    e2["ub"][1] = e2["key"][1] + (ents["ub"][1] - ents["key"][1])
    with pytest.raises(AssertionError, match="K_s"):
        cc.check(corpus, Q, recs, e2, 0, dists=dists, sketch=sketch)
    # D: above what thr_min implies
    r3 = recs.copy()
    r3["D"][0] = r3["D"][0] * 1.001 + 1e-6
    r3["certified"][0] = 0
    with pytest.raises(AssertionError, match="D: "):
        cc.check(corpus, Q, r3, ents, 0, dists=dists, sketch=sketch)
    # S: D - slack beyond a left-out row
    r4 = recs.copy()
    r4["certified"][:] = 1
    r4["slack"][:] = -1e9 if metric == 0 else -2.0
    with pytest.raises(AssertionError, match="S: "):
        cc.check(corpus, Q, r4, ents, 0, dists=dists)
