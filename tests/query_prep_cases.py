"""Shared by test_query_prep_cpu.py and test_gpu_query_prep.py: the query vectors that the 8-bit query rule
(syzgydb_amd/csrc/query_prep.h) can go wrong on, and the rule restated in Python floats and ints -- not a line of the
header: IEEE doubles one operation at a time (numpy's float64 scalars, which overflow and divide as the hardware does
where Python's floats raise), Python's unbounded ints for the digits."""
import math
import struct

import numpy as np

NAMES = ("normal", "normal_small", "zero", "nan", "pos_inf", "neg_inf", "all_equal", "signed_zero_subnormal", "huge",
         "single_nonzero", "single_negative", "ties", "digit_borrow")

# On a Euclidean handle the prepared query is 255 q; with a largest element of Qmax the step is (255 Qmax) / Qmax = 255
# exactly, so v / qs is q itself wherever 255 q is exact: q = n + 1/2 lands ON the tie, its neighbours in the last place
# beside it.  (Under cosine the same vectors are merely odd; the CPU test's Python rule says what is right there too.)
_HALVES = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 63.5, -63.5, 64.5, -64.5, 127.5, -127.5, 128.5, -128.5, 8191.5, -8192.5]
# negative (and positive) Q of every digit pattern class of the balanced split: low digit at and beside -64 / 63, a borrow
# into the m digit, into the h digit, the clamp
_DIGITS = [-1, 1, -63, 63, -64, 64, -65, 65, -127, -128, -129, 127, 128, 129, -8128, -8129, 8127, 8128, -8191, -8192, -8193,
           8191, 8192, 8193, -15999, -16000, -16001, -16383, -16384, -16385, 16383, 16384, 16385, -999999, -1000000, 123456,
           -123456, -524288, 524287]


def _place(dim, head, values):
    """head first (the element that fixes the step), then the values as far as dim reaches, the rest zero"""
    v = np.zeros(dim)
    seq = [head] + list(values)
    v[: min(dim, len(seq))] = seq[:dim]
    return v


def vectors(dim, planes, seed):
    """{name: float64[dim]}: every class of the list in the option's issue, at this dimension."""
    rng = np.random.default_rng(seed)
    qmax = 16000.0 if planes == 2 else 1000000.0
    out = {}
    out["normal"] = rng.standard_normal(dim)
    out["normal_small"] = rng.standard_normal(dim) * 1e-3
    out["zero"] = np.zeros(dim)
    v = rng.standard_normal(dim)
    v[dim // 2] = np.nan
    out["nan"] = v
    v = rng.standard_normal(dim)
    v[dim - 1] = np.inf
    out["pos_inf"] = v
    v = rng.standard_normal(dim)
    v[0] = -np.inf
    out["neg_inf"] = v
    out["all_equal"] = np.full(dim, -0.37)
    tiny = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -1e-310, 1e-320, -0.0]
    out["signed_zero_subnormal"] = np.array([tiny[i % len(tiny)] for i in range(dim)])
    v = rng.standard_normal(dim) * 1e300   # (m1 overflows to +inf)
    out["huge"] = v
    v = np.zeros(dim)
    v[dim // 3] = 3.25
    out["single_nonzero"] = v
    v = np.zeros(dim)
    v[dim - 1] = -7e-5
    out["single_negative"] = v
    ties = []
    for h in _HALVES:
        ties += [h, np.nextafter(h, 0.0), np.nextafter(h, math.copysign(np.inf, h))]
    out["ties"] = _place(dim, qmax, ties)
    out["digit_borrow"] = _place(dim, -qmax, [float(x) for x in _DIGITS if abs(x) <= qmax])   # (beyond Qmax they would set the step)
    assert tuple(out) == NAMES
    return out


def batch(dim, planes, seed, n):
    """n queries: the special vectors in turn, then normal draws of growing scale"""
    special = list(vectors(dim, planes, seed).values())
    rng = np.random.default_rng(seed + 1)
    rows = [special[i] if i < len(special) else rng.standard_normal(dim) * 10.0 ** (i % 7 - 3) for i in range(n)]
    return np.stack(rows)


# ---- the rule, restated -------------------------------------------------------------------------------------------------

def _round_clamp(t, lim):
    if t != t:
        return 0
    t = min(max(t, -lim), lim)
    return int(t + (0.5 if t >= 0 else -0.5))   # (int() truncates toward zero, as the C cast does)


def prepare(q, cosine, planes, gs=0.0):
    """-> (image bytes, (qnorm, m1, qscale, qconst, qnorm2)) of one query of an 8-bit index"""
    q = [float(x) for x in q]
    if gs > 0.0:
        q = [float(np.float64(x) / np.float64(gs)) for x in q]   # (IEEE division; a zero divisor never gets here)
    dim = len(q)
    with np.errstate(all="ignore"):
        f = np.float64
        m1 = f(0.0)
        for x in q:
            m1 = m1 + f(x) * f(x)
        if cosine:
            scale = f(1.0) / np.sqrt(m1) if m1 > 0 else f(0.0)
        else:
            scale = f(255.0)
        nrm, vmax = f(0.0), f(0.0)
        vs = []
        for x in q:
            v = f(x) * scale
            vs.append(v)
            nrm = nrm + v * v
            a = abs(v)
            if vmax < a:          # (std::max(vmax, a): a NaN never enters)
                vmax = a
        qmax = f(16000.0 if planes == 2 else 1000000.0)
        qs = vmax / qmax if (vmax > 0 and np.isfinite(vmax)) else f(1.0)
        r16 = (dim + 15) // 16
        image = bytearray(48 * r16)
        total = 0
        for e, v in enumerate(vs):
            Q = _round_clamp(float(v / qs), float(qmax))
            total += Q
            rest = Q
            for x in range(2, 2 - planes, -1):
                if x > 3 - planes:
                    dig = ((rest + 64) & 127) - 64
                    rest = (rest - dig) >> 7
                else:
                    dig = rest
                assert -128 <= dig <= 127, (Q, x, dig)
                word = (x * r16 + e // 16) * 4 + (e % 16) // 4
                image[word * 4 + (e % 16) % 4] = dig & 0xFF
        meta = (float(np.sqrt(nrm)), float(m1), float(qs), float(total), float(nrm))
    return bytes(image), meta


def bits(x):
    """the float64's bit pattern; a NaN constant is THE quiet NaN, whatever sign and payload the arithmetic left it"""
    return 0x7FF8000000000000 if x != x else struct.unpack("<Q", struct.pack("<d", x))[0]
