"""The certificate of the sketch-on-sketch join (szg_index_neighbors) evaluated on the CPU, no device: a numpy model of the
8-bit sketch (cert_check.sketch_reference, sketch_slack) and float64 distances decide, for every row of a collection as
the query, whether   d_k (1 + 1e-9) < D_lb - 2 slack   holds with D_lb from the kp-th best sketch-to-sketch key.  The
slices' drop bounds and the key bound (at most 6 * 2^-24) are left out: the model is an upper bound on what settles.

    python scripts/neighbors_model.py            # the shapes of tests/test_gpu_neighbors.py, plain and clustered rows

One line per shape: rows the model hands over of all rows as queries (profiles/neighbors.txt keeps the table)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from syzgydb_amd import cert_check as cc, SZG_COSINE, SZG_EUCLIDEAN  # noqa: E402


def vectors(n, dim, seed, clustered):
    g = np.random.default_rng(seed)
    if not clustered:
        return g.standard_normal((n, dim))
    centers = g.standard_normal((max(1, n // 20), dim))
    return centers[np.arange(n) % centers.shape[0]] + 0.3 * g.standard_normal((n, dim))


def handed_over(vec, metric, k, bits=32):
    X = vec.astype(np.float32).astype(np.float64) if bits == 32 else vec
    n, dim = X.shape
    gs = 0.0 if metric == SZG_COSINE else float(np.abs(X).max())
    t, must = cc.sketch_reference(X, metric, gs)
    assert not must.any()
    N = 2.0 * np.clip(np.rint(t.astype(np.float64)), 0, 255) - 255.0
    kk = k + 30
    kp = kk + max(16, kk // 2)
    if metric == SZG_COSINE:
        def dist(A, B):
            c = (A @ B.T) / np.sqrt((A * A).sum(1)[:, None] * (B * B).sum(1)[None, :])
            return np.arccos(np.clip(c, -1.0, 1.0)) / np.pi
        own = np.arccos(np.clip((X * N).sum(1) / np.sqrt((X * X).sum(1) * (N * N).sum(1)), -1, 1)) / np.pi
        d_sk = dist(N, N)
    else:
        def dist(A, B):
            return np.sqrt(np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2 * A @ B.T, 0.0))
        S = gs * N / 255.0
        own = np.sqrt(((X - S) ** 2).sum(1))
        d_sk = dist(S, S)
    slack = cc.sketch_slack(float(own.max()), gs, dim)
    d_k = np.sort(dist(X, X), axis=1)[:, k - 1]
    D_lb = np.sort(d_sk, axis=1)[:, min(kp, n) - 1]
    return int((~(d_k * (1 + 1e-9) < D_lb - 2 * slack)).sum()), n, slack


if __name__ == "__main__":
    shapes = [(SZG_COSINE, 64, 16 * 70 - 1, 10), (SZG_EUCLIDEAN, 192, 16 * 70, 1), (SZG_COSINE, 768, 16 * 125 + 1, 10),
              (SZG_EUCLIDEAN, 768, 16 * 125 + 1, 10), (SZG_EUCLIDEAN, 1088, 16 * 100 - 1, 10), (SZG_COSINE, 2112, 16 * 64 + 1, 10),
              (SZG_COSINE, 192, 16 * 70, 10), (SZG_EUCLIDEAN, 192, 16 * 140, 10)]
    for metric, dim, n, k in shapes:
        for clustered in (False, True):
            bad, n_, slack = handed_over(vectors(n, dim, 3, clustered), metric, k)
            print("metric %d dim %4d rows %4d k %2d %-9s handed over %4d of %4d  (2 slack = %.3g)" % (
                metric, dim, n, k, "clustered" if clustered else "plain", bad, n_, 2 * slack), flush=True)
