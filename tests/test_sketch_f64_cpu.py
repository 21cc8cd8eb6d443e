"""The 8-bit sketch of float64 rows (option sketch_f64), without a device.

tests/test_gpu_sketch_f64.py holds the card's sketch of double rows against cert_check.check_sketch_build.  Here the
sketch is made with numpy two ways -- from the double values, as sketch_build_f64_kernel is specified (every element
times 2^-e, e the binary exponent of the scale, then byte = clip(rint((y / m + 1) * 127.5), 0, 255)), and from the rows
narrowed to float32 first, as the float32 kernel's arithmetic would see them -- so that

  * the option's value range is the library's own (szg_debug_option_check),
  * the checks pass on the sketch made from the doubles, at magnitudes float32 cannot hold, and
  * they raise on the sketch made from narrowed rows (a row of 1e-60 loses its direction, a row of 1e60 becomes
    infinite, a row whose largest element is subnormal becomes zero), and on one made with 1 / max|x_i|, which
    overflows for that last row.
"""
import numpy as np
import pytest

from syzgydb_amd import SzgError, _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import option_check

EUC, COS = 0, 1
DIM, N = 24, 64
ALT = np.where(np.arange(DIM) % 3 == 0, -1.0, 1.0)


def test_option_values():
    """sketch_f64 is 0 or 1: the hook answers as szg_set_option would."""
    for v in (0, 1):
        option_check("sketch_f64", v)
    for v in (2, -1):
        with pytest.raises(SzgError, match="sketch_f64 is 0 or 1") as e:
            option_check("sketch_f64", v)
        assert e.value.code == _lib.SZG_E_INVALID


def sketch_of(X, metric, how):
    """Row values X[n, dim] (float64) -> (bytes, info, exc_rows) as a full rebuild would leave them.

    how: "f64"        the double kernel's arithmetic (power-of-two scaling, no narrowing)
         "narrowed"   the rows narrowed to float32 first, then the float32 kernel's arithmetic
         "reciprocal" the doubles, but scaled by 1.0 / scale as the float32 kernel scales"""
    with np.errstate(all="ignore"):
        V = X.astype(np.float32).astype(np.float64) if how == "narrowed" else X
        fin = np.isfinite(V).all(axis=1)
        mx = np.abs(np.where(np.isfinite(V), V, 0.0)).max(axis=1)
        if metric == COS:
            gscale, bad = 0.0, ~fin | (mx == 0)
            scale = np.where(bad, 1.0, mx)
        else:
            gscale = float(mx[fin].max()) if fin.any() and mx[fin].max() > 0 else 1.0
            bad = ~fin | (mx > gscale)
            scale = np.full(V.shape[0], gscale)
        if how == "f64":
            m, e = np.frexp(scale)
            Y = np.ldexp(V, -e[:, None])
            t = (Y * (1.0 / m)[:, None] + 1.0) * 127.5
        else:
            Y, m, e = V, scale, np.zeros(V.shape[0], dtype=np.int64)
            t = (V * (1.0 / scale)[:, None] + 1.0) * 127.5
        v = np.clip(np.rint(np.where(np.isnan(t), 127.5, t)), 0, 255)
        v[bad] = 128
        v = v.astype(np.uint8)
        nvec = 2.0 * v[~bad] - 255.0
        Yk, mk, ek = Y[~bad], m[~bad], e[~bad]
        if gscale > 0:
            d = np.ldexp(np.sqrt(((Yk - mk[:, None] * nvec / 255.0) ** 2).sum(axis=1)), ek)
        else:
            c = (Yk * nvec).sum(axis=1) / np.sqrt((Yk ** 2).sum(axis=1) * (nvec ** 2).sum(axis=1))
            d = np.arccos(np.clip(c, -1, 1)) / np.pi
        d = d[np.isfinite(d)]
    exc = np.flatnonzero(bad).astype(np.uint64)
    info = {"exists": 1, "in_sync": 1, "disabled": 0, "rows": X.shape[0], "max_ang": float(d.max()) if d.size else 0.0,
            "gscale": gscale, "n_exc": exc.size}
    return v, info, exc


def rows(factor):
    """Ordinary rows times `factor`; row 5 has every |x_i| equal."""
    rng = np.random.default_rng(0xF64)
    X = rng.uniform(-1.0, 1.0, (N, DIM)) * factor
    X[5] = 0.75 * ALT * factor
    return X


def subnormal_rows():
    """Ordinary rows, and row 7 whose largest element is 1e-320, a subnormal double."""
    X = rows(1.0)
    X[7] = ALT * 1e-320 * (1 + np.arange(DIM) % 3) / 3.0
    return X


CASES = {"1e-60": lambda: rows(1e-60), "1e60": lambda: rows(1e60), "subnormal": subnormal_rows}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cosine_sketch_needs_the_double_values(name):
    X = CASES[name]()
    v, info, exc = sketch_of(X, COS, "f64")
    got = cc.check_sketch_build(X, v, info, exc, True, metric=COS, what=(name,))
    assert got["sketched"] == N and exc.size == 0 and 0 < got["share"] <= 1.0
    # narrowed to float32: a row without a direction (1e-60, the subnormal row) or with infinite elements (1e60) is an
    # exception that need not be one (B2) -- or, not listed, its bytes of 128 are not the nearest (B1)
    v32, info32, exc32 = sketch_of(X, COS, "narrowed")
    assert exc32.size == (1 if name == "subnormal" else N)
    with pytest.raises(AssertionError, match="B2"):
        cc.check_sketch_build(X, v32, info32, exc32, True, metric=COS, what=(name,))
    with pytest.raises(AssertionError, match="B1"):
        cc.check_sketch_build(X, v32, dict(info32, n_exc=0), exc32[:0], True, metric=COS, what=(name,))


def test_reciprocal_of_a_subnormal_scale_overflows():
    """1.0 / 1e-320 is infinite: every byte of the row clips to 0 or 255.  B1 sees it; dividing (or a power of two) does not."""
    X = subnormal_rows()
    v, info, exc = sketch_of(X, COS, "reciprocal")
    assert set(int(b) for b in v[7]) <= {0, 255}
    with pytest.raises(AssertionError, match="B1"):
        cc.check_sketch_build(X, v, info, exc, True, metric=COS)
    v, info, exc = sketch_of(X, COS, "f64")
    assert set(int(b) for b in v[7]) == {85, 212, 255}   # (-1/3, 2/3 and 1 times the scale)
    cc.check_sketch_build(X, v, info, exc, True, metric=COS)


@pytest.mark.parametrize("factor", (1e-60, 1e60, 1e200))
def test_euclidean_sketch_needs_the_double_values(factor):
    """One scale for the collection: at 1e200 the squares of the differences overflow a double unless they are summed in
    units of the scale."""
    X = rows(factor)
    v, info, exc = sketch_of(X, EUC, "f64")
    assert info["gscale"] == np.abs(X).max() and np.isfinite(info["max_ang"]) and info["max_ang"] > 0
    got = cc.check_sketch_build(X, v, info, exc, True, metric=EUC, what=(factor,))
    assert got["sketched"] == N and got["share"] <= 1.0
    v32, info32, exc32 = sketch_of(X, EUC, "narrowed")
    with pytest.raises(AssertionError, match="B1|B2|scale"):
        cc.check_sketch_build(X, v32, info32, exc32, True, metric=EUC, what=(factor,))
