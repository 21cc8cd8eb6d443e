"""The 8-bit sketch pre-pass on float64 rows, the reference's default quantization (option sketch_f64).

Handles hold 64-bit rows and are opened with sketch_f64 = 1, sketch = 1, sketch_min_rows = 1, multi_query = 0 and the
certificate trace on.  Every link of the chain that makes a sketch answer exact is held against float64,
as tests/test_gpu_sketch_state.py holds it for float32 rows:

    1  the build kernel for double rows (sketch_build_f64_kernel): check_sketch_build's B1 .. B4 and the Euclidean scale
       at magnitudes only doubles have -- per-row factors of 1e-150 .. 1e150, a largest element of 1e-320 (1 / max
       overflows), an element of 1.7e308 (its square overflows), a collection at 1e200 (the square of a Euclidean
       difference overflows)
    2  the float32 path as the yardstick: values a float32 row holds, loaded into a 32-bit handle and, as doubles, into a
       64-bit one, give the same sketch bytes, max_ang, scale, exceptions, certificate records and answers
    3  a corpus no float32 handle can hold: answers, K_s, L_s, D and S
    4  the state through overwrites, appends, tombstones and compaction; the option left at 0 and set back to 0
    5  radius searches (sketch_radius) and masked launches (sketch_masked) through the sketch of double rows

tests/test_sketch_f64_cpu.py shows without a device that the build checks reject a sketch made from narrowed rows."""
import numpy as np
import pytest

import oracle as orc
import test_gpu_sketch_state as tss
from syzgydb_amd import ScanIndex, _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import pack_allow_bits, scan_masked_plan

pytestmark = pytest.mark.gpu

SEED = 0x53595A470000F640
EUC, COS = 0, 1
MID = {EUC: "euc", COS: "cos"}
POOL = tss.POOL
DBL_MAX = float(np.finfo(np.float64).max)


def open64(dim, metric, f64=1, **options):
    ix = ScanIndex(dim, 64, metric)
    for name, value in dict({"sketch_f64": f64, "sketch": 1, "sketch_min_rows": 1, "multi_query": 0}, **options).items():
        ix.set_option(name, value)
    ix.trace_certificates(True)
    return ix


def same(g, w):
    g, w = np.asarray(g), np.asarray(w)
    return g.shape == w.shape and bool(((g == w) | (np.isnan(g) & np.isnan(w))).all())


def assert_answers(got, packed, dim, bits, metric, Q, k, eligible, what):
    r, d, cnt = got
    allow = None if eligible is None else eligible.astype(np.uint8)
    want = POOL.map(lambda q: orc.search_exact(packed, dim, bits, metric, q, k=k, allow=allow)[:2], Q)
    for qi, (w_rows, w_dist) in enumerate(want):
        assert [int(x) for x in r[qi, : cnt[qi]]] == [int(x) for x in w_rows], ("rows differ", what, qi)
        assert same(d[qi, : cnt[qi]], w_dist), ("distances not bit-equal", what, qi)


def searched_state(ix, packed, metric, Q, rebuilt, live, what, k=10):
    """One search, then B on the state it left (test_gpu_sketch_state.searched_state, for 64-bit rows)."""
    dim = ix.dim
    got = ix.search_topk(Q, k)
    recs, _, dropped = ix.certificates()
    sk = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]
    assert dropped == 0 and sorted(int(x) for x in sk["query"]) == list(range(Q.shape[0])), ("one sketch record per query", what)
    info = ix.sketch_info()
    assert info["exists"] == 1 and info["in_sync"] == 1 and info["disabled"] == 0, (what, info)
    assert info["rows"] == packed.shape[0], (what, info)
    sk_bytes, words = ix.sketch_rows()
    assert sk_bytes.shape == (packed.shape[0], dim), (what, sk_bytes.shape)
    assert np.isfinite(info["max_ang"]) and info["max_ang"] >= 0, (what, info)
    out = cc.check_sketch_build(cc.decode_rows(packed, dim, 64), sk_bytes, info, info["exc_rows"], rebuilt, metric=metric,
                                rec_slack=sk["slack"][0], what=what)
    want = pack_allow_bits(np.ones(packed.shape[0], dtype=bool) if live is None else live)[0]
    assert (words == want).all(), ("the sketch shards' live words are not the rows'", what)
    assert out["share"] <= 1.0
    assert_answers(got, packed, dim, 64, metric, Q, k, live, what)
    return out


# ---- 1. the build kernel for double rows ------------------------------------------------------------------------------------

BUILD_DIMS = (1, 3, 15, 16, 17, 63, 64, 65, 768, 1025)
BUILD_ROWS = 1501   # not a multiple of the 4 waves (rows) of a block
BAD_AT = tss.BAD_AT   # rows 17 .. 22: Inf / NaN at the first, middle and last element
R_ONE, R_EQUAL, R_ZERO, R_TINY, R_HUGE, R_PAIR = 10, 11, 12, 23, 24, 25


def build_rows(dim, metric):
    """test_gpu_sketch_state.build_rows with the factors doubles allow -- 1e-150 .. 1e150 under cosine (each row its own
    scale), 1e-3 .. 1e3 under Euclid (one scale) -- and hand-made rows."""
    n = BUILD_ROWS
    rng = np.random.default_rng(dim * 2 + metric)
    span = 150.0 if metric == COS else 3.0
    vec = orc.synth_vectors(SEED + dim, 0, n, dim) * 10.0 ** rng.permutation(np.linspace(-span, span, n))[:, None]
    alt = np.where(np.arange(dim) % 3 == 0, -1.0, 1.0)
    vec[R_ONE] = 0.0
    vec[R_ONE, dim - 1] = -2.5                            # one non-zero element
    vec[R_EQUAL] = 0.75 * alt                             # every |x_i| equal: the sketch is exact, the angle 0
    vec[R_ZERO] = 0.0 * alt                               # +-0.0 only: no direction
    for name, r in BAD_AT.items():
        at = {"first": 0, "last": dim - 1, "middle": dim // 2}[name.split()[1]]
        vec[r, at] = {"inf": np.inf, "-inf": -np.inf, "nan": np.nan}[name.split()[0]]
    vec[R_TINY] = alt * 1e-320 * (1 + np.arange(dim) % 3) / (3.0 if dim >= 3 else 1.0)   # the largest element is 1e-320
    assert np.abs(vec[R_TINY]).max() == 1e-320
    if metric == COS:
        vec[R_HUGE, dim // 2] = 1.7e308                   # (Euclid: appended later -- it becomes the scale of every row)
    vec[R_PAIR] = orc.synth_vectors(SEED + dim + 7, 0, 1, dim)[0]
    vec[R_PAIR + 1] = vec[R_PAIR] * (1.0 + 1e-10 * (1 + np.arange(dim) % 2))   # the neighbour, below float32's resolution
    with np.errstate(all="ignore"):   # (an element within 2e-10 of a float32 rounding edge may part them: one in 300)
        assert (vec[R_PAIR + 1] != vec[R_PAIR]).all()
        assert (vec[R_PAIR + 1].astype(np.float32) == vec[R_PAIR].astype(np.float32)).mean() >= 0.98
    return vec


@pytest.mark.parametrize("metric", (EUC, COS), ids=["euc", "cos"])
@pytest.mark.parametrize("dim", BUILD_DIMS)
def test_build_kernel(dim, metric):
    """B after a search of 2 queries, again after an overwrite and after an append: a lone short piece whose last 16 bytes
    hold one double (1, 3, 15), whole and ragged pieces (16, 17, 63 .. 65), 768, a second piece on lane 0 (1025)."""
    vec = build_rows(dim, metric)
    packed = orc.encode_rows(vec, 64)
    assert same(cc.decode_rows(packed, dim, 64), vec)
    Q = orc.synth_vectors(SEED + dim + 1, 0, 2, dim)
    what = ("build", dim, MID[metric])
    bad = set(BAD_AT.values())
    want_exc = bad | {R_ZERO} if metric == COS else bad
    with open64(dim, metric) as ix:
        ix.load(packed)
        assert ix.sketch_info()["exists"] == 0
        out = searched_state(ix, packed, metric, Q, True, None, what)
        assert set(int(r) for r in ix.sketch_info()["exc_rows"]) == want_exc, what
        assert out["sketched"] == BUILD_ROWS - len(want_exc)
        # an overwrite (the float64 entry point): only the listed row is built
        far = np.full(dim, 1e-6)
        far[0] = 0.9
        packed[40] = orc.encode_rows(far[None, :], 64)[0]
        ix.overwrite_vector(40, far)
        assert ix.sketch_info()["in_sync"] == 0
        searched_state(ix, packed, metric, Q, False, None, what + ("overwrite",))
        # an append: only the new rows are built
        more = orc.synth_vectors(SEED + dim + 2, 0, 3, dim) * np.array([1e-2, 1.0, 0.5])[:, None]
        more[1] = more[0] * (1.0 + 1e-10)
        packed = np.concatenate([packed, orc.encode_rows(more, 64)])
        ix.append(packed[-3:])
        assert ix.sketch_info()["in_sync"] == 0
        searched_state(ix, packed, metric, Q, False, None, what + ("append",))
        assert set(int(r) for r in ix.sketch_info()["exc_rows"]) == want_exc, what
        if metric == EUC:   # a double near the largest becomes the one scale: a rebuild, the scale exact
            top = np.zeros((1, dim))
            top[0, dim // 2] = -1.7e308
            packed = np.concatenate([packed, orc.encode_rows(top, 64)])
            ix.append(packed[-1:])
            searched_state(ix, packed, metric, Q, True, None, what + ("largest double",))
            info = ix.sketch_info()
            assert info["gscale"] == 1.7e308 and set(int(r) for r in info["exc_rows"]) == bad, (what, info)
            assert info["max_ang"] <= DBL_MAX


def test_euclid_every_row_times_1e200():
    """The square of a Euclidean difference overflows at this scale: the state is a valid sketch or a clean step aside,
    max_ang is finite either way, and the answers are the oracle's (whose own distances overflow: every query ties)."""
    dim, n = 64, BUILD_ROWS
    vec = orc.synth_vectors(SEED + 900, 0, n, dim) * 1e200
    packed = orc.encode_rows(vec, 64)
    Q = orc.synth_vectors(SEED + 901, 0, 3, dim) * 1e200
    what = ("1e200",)
    with open64(dim, EUC) as ix:
        ix.load(packed)
        got = ix.search_topk(Q, 10)
        recs, _, _ = ix.certificates()
        info = ix.sketch_info()
        assert np.isfinite(info["max_ang"]) and np.isfinite(info["gscale"]), info
        if info["exists"]:
            assert info["in_sync"] == 1 and info["disabled"] == 0, info
            sk = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]
            assert len(sk) == 3 and np.isfinite(sk["slack"]).all(), sk
            out = cc.check_sketch_build(vec, ix.sketch_rows()[0], info, info["exc_rows"], True, metric=EUC,
                                        rec_slack=sk["slack"][0], what=what)
            assert out["sketched"] == n and info["gscale"] == np.abs(vec).max()
        else:
            assert info["disabled"] == 1, info
        assert_answers(got, packed, dim, 64, EUC, Q, 10, None, what)


# ---- 2. the float32 path is the yardstick -------------------------------------------------------------------------------------

REC_FIELDS = ("thr_min", "D", "slack", "certified")


def sketch_records(ix, nq):
    recs, _, dropped = ix.certificates()
    sk = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]
    assert dropped == 0 and sorted(int(x) for x in sk["query"]) == list(range(nq))
    return sk[np.argsort(sk["query"], kind="stable")]


@pytest.mark.parametrize("metric", (EUC, COS), ids=["euc", "cos"])
@pytest.mark.parametrize("dim", (64, 100))
def test_twin_of_a_float32_handle(dim, metric):
    """Values a float32 row holds exactly, as a 32-bit and as a 64-bit handle: the sketch state, every sketch record and
    every answer are the same, through the lone (1), grouped or matrix (3, 16), two-block (17) and shared (33) forms --
    dim 100 is untiled and keeps the grouped kernel."""
    n = 3000
    packed32 = orc.synth_rows(SEED + dim, 0, n, dim, 32)
    X = cc.decode_rows(packed32, dim, 32)
    packed64 = orc.encode_rows(X, 64)
    assert same(cc.decode_rows(packed64, dim, 64), X)
    Qall = orc.synth_vectors(SEED + dim + 1, 0, 33, dim) * 0.7
    forms = {"sketch_wide": 2, "sketch_share": 2}
    with tss.open_sketched(dim, metric, **forms) as ix32, open64(dim, metric, **forms) as ix64:
        ix32.load(packed32)
        ix64.load(packed64)
        first = True
        for k in (1, 10):
            settled = total = 0
            for nq in (1, 3, 16, 17, 33):
                what = ("twin", dim, MID[metric], "k", k, "queries", nq)
                Q = Qall[:nq]
                got32, got64 = ix32.search_topk(Q, k), ix64.search_topk(Q, k)
                r32, r64 = sketch_records(ix32, nq), sketch_records(ix64, nq)
                settled += int((r32["certified"] == 1).sum())   # (on the yardstick's side)
                total += nq
                for f in REC_FIELDS:
                    assert same(r32[f], r64[f]), ("sketch records differ", what, f, r32[f][:4], r64[f][:4])
                for a, b in zip(got32, got64):
                    assert same(a, b), ("answers differ between the handles", what)
                assert_answers(got64, packed64, dim, 64, metric, Q, k, None, what)
                if first:
                    first = False
                    i32, i64 = ix32.sketch_info(), ix64.sketch_info()
                    assert i32["in_sync"] == 1 and i64["in_sync"] == 1
                    for f in ("rows", "max_ang", "gscale", "n_exc"):
                        assert i32[f] == i64[f], ("sketch state differs", what, f, i32[f], i64[f])
                    assert (i32["exc_rows"] == i64["exc_rows"]).all()
                    assert (ix32.sketch_rows()[0] == ix64.sketch_rows()[0]).all(), ("sketch bytes differ", what)
            assert 2 * settled >= total, ("the float32 handle settled too few queries: two fallbacks would be compared", dim, k, settled, total)
        s32, s64 = ix32.stats(), ix64.stats()
        for f in ("sketch_queries", "sketch_fallbacks"):
            assert s32[f] == s64[f], (f, s32[f], s64[f])
        assert s64["sketch_queries"] > 0


# ---- 3. a corpus only doubles hold ----------------------------------------------------------------------------------------------

def double_only_rows(dim, metric):
    """800 rows x, their 800 partners -- the first 100 x (1 + 1e-10), the rest x_i (1 + 1e-10 g_i) -- and 800 more rows.
    Cosine: the 800 are at 1e-60 beside the others at 1.  Euclid has one scale for the collection, and rows at 1e-60
    beside rows at 1 would all sit at the origin, every one of them at the same distance from a query (ties, which are
    the full sweep's): there the whole corpus is at 1e-60, the 800 included."""
    base = orc.synth_vectors(SEED + 3000 + dim, 0, 1600, dim)
    x, rest = base[:800], base[800:]
    g = np.random.default_rng(dim).uniform(-1.0, 1.0, x.shape)
    g[:100] = 1.0
    partner = x * (1.0 + 1e-10 * g)
    assert (partner.astype(np.float32) == x.astype(np.float32)).mean() > 0.99   # (no float32 twin tells them apart)
    if metric == EUC:
        return np.concatenate([x, partner, rest]) * 1e-60
    return np.concatenate([x, partner, rest * 1e-60])


@pytest.mark.parametrize("metric", (EUC, COS), ids=["euc", "cos"])
def test_double_only_corpus(metric):
    dim, k, nq = 64, 10, 12
    vec = double_only_rows(dim, metric)
    corpus = cc.Corpus(orc.encode_rows(vec, 64), dim, 64, metric)
    Q = orc.synth_vectors(SEED + 3100, 0, nq, dim) * 0.7 * (1e-60 if metric == EUC else 1.0)
    what = ("double only", MID[metric])
    with open64(dim, metric) as ix:
        ix.load(corpus.packed)
        got = ix.search_topk(Q, k)
        recs, ents, dropped = ix.certificates()
        sk = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]
        assert sorted(int(x) for x in sk["query"]) == list(range(nq)), ("one sketch record per query", what)
        info = ix.sketch_info()
        assert info["in_sync"] == 1 and info["n_exc"] == 0, (what, info)
        sk_bytes = ix.sketch_rows()[0]
        cc.check_sketch_build(vec, sk_bytes, info, info["exc_rows"], True, metric=metric, rec_slack=sk["slack"][0], what=what)
        sk_corpus = cc.Corpus(sk_bytes, dim, 8, metric)
        dists = np.stack(list(POOL.map(lambda q: orc.all_distances(corpus.packed, dim, 64, metric, q), Q)))
        s = cc.check(corpus, Q, recs, ents, dropped, dists=dists, what=what,
                     sketch=(sk_corpus, info["gscale"], info["exc_rows"]))
        assert s.checked > 0, ("no key was checked", what)
        assert_answers(got, corpus.packed, dim, 64, metric, Q, k, None, what)
        st = ix.stats()
        print(what, "settled", st["sketch_queries"], "handed over", st["sketch_fallbacks"])
        assert st["sketch_queries"] + st["sketch_fallbacks"] == nq and st["sketch_queries"] == int((sk["certified"] == 1).sum())
        assert st["sketch_queries"] > st["sketch_fallbacks"], (what, st)


# ---- 4. the state through mutations ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", (EUC, COS), ids=["euc", "cos"])
def test_lifecycle(metric):
    dim, n0 = 48, 2000
    pool = orc.synth_vectors(SEED + 4000 + metric, 0, n0 + 400, dim)
    fresh = pool[n0 + 100:] * 0.9   # (inside the Euclidean scale: no step below is a rebuild but the ones marked)
    Q = orc.synth_vectors(SEED + 4001, 0, 3, dim) * 0.7
    what = ("lifecycle", MID[metric])
    with open64(dim, metric) as ix:
        vec = pool[:n0].copy()
        packed = orc.encode_rows(vec, 64)
        ix.load(packed)

        def step(name, rebuilt, live=None, rows=None):
            info = ix.sketch_info()
            assert info["in_sync"] == 0, (what, name, "before the search", info)
            searched_state(ix, packed, metric, Q, rebuilt, live, what + (name,))
            info = ix.sketch_info()
            assert (info["in_sync"], info["rows"]) == (1, packed.shape[0] if rows is None else rows), (what, name, info)

        step("load", True)
        packed[5] = orc.encode_rows(fresh[:1], 64)[0]
        ix.overwrite(5, packed[5])
        step("overwrite", False)
        packed[6] = orc.encode_rows(fresh[1:2], 64)[0]
        ix.overwrite_vector(6, fresh[1])
        step("overwrite_vector", False)
        at = np.arange(100, 150)
        packed[at] = orc.encode_rows(fresh[2:52], 64)
        ix.overwrite_rows(at, packed[at])
        step("overwrite_rows", False)
        at = np.arange(300, 350)
        packed[at] = orc.encode_rows(fresh[52:102], 64)
        ix.overwrite_vectors(at, fresh[52:102])
        step("overwrite_vectors", False)
        packed = np.concatenate([packed, orc.encode_rows(pool[n0:n0 + 100] * 0.9, 64)])
        ix.append(packed[n0:])
        step("append", False)
        n = packed.shape[0]
        live = np.ones(n, dtype=bool)
        live[np.arange(3, n, 70)] = False
        ix.tombstone_rows(np.flatnonzero(~live))
        step("tombstones", False, live)
        ix.compact()
        packed = packed[live]
        step("compact", True)
        st = ix.stats()
        assert st["sketch_queries"] + st["sketch_fallbacks"] == 8 * 3 and st["sketch_queries"] > 0, (what, st)
        # set back to 0: the handle's own path, the sketch index left as "sketch" = 0 leaves a float32 handle's
        ix.set_option("sketch_f64", 0)
        ix.reset_stats()
        got = ix.search_topk(Q, 10)
        st = ix.stats()
        assert st["sketch_queries"] + st["sketch_fallbacks"] == 0 and st["scan_launches"] >= 1, (what, st)
        assert ix.sketch_info()["exists"] == 1   # (kept, as a float32 handle keeps its sketch index under sketch = 0)
        assert_answers(got, packed, dim, 64, metric, Q, 10, None, what + ("set back to 0",))
        ix.set_option("sketch_f64", 1)
        ix.search_topk(Q, 10)
        assert ix.stats()["sketch_queries"] + ix.stats()["sketch_fallbacks"] == 3


def test_option_off_keeps_no_sketch():
    """sketch = 1 on a 64-bit handle with sketch_f64 left at 0: no sketch index, no query through one."""
    dim, n = 48, 2000
    packed = orc.encode_rows(orc.synth_vectors(SEED + 4100, 0, n, dim), 64)
    Q = orc.synth_vectors(SEED + 4101, 0, 3, dim) * 0.7
    with open64(dim, COS, f64=0, sketch_radius=1) as ix:   # (0 is what a handle that never heard of the option has)
        ix.load(packed)
        got = ix.search_topk(Q, 10)
        ix.search_radius(Q[0], 0.4)
        info, st = ix.sketch_info(), ix.stats()
        assert info["exists"] == 0 and info["rows"] == 0, info
        assert st["sketch_queries"] == 0 and st["sketch_fallbacks"] == 0 and st["sketch_radius_queries"] == 0, st
        assert_answers(got, packed, dim, 64, COS, Q, 10, None, ("option off",))


# ---- 5. radius searches and masked launches -------------------------------------------------------------------------------------

def radius_at(d, m):
    """The midpoint between the m-th and the (m + 1)-th smallest distance: no predicate sits on a rounding edge."""
    s = np.sort(d[np.isfinite(d)])
    r = float((s[m - 1] + s[m]) / 2)
    assert s[m - 1] < r < s[m]
    return r


@pytest.mark.parametrize("metric", (EUC, COS), ids=["euc", "cos"])
def test_radius_through_the_sketch(metric):
    dim, n = 64, 3000
    packed = orc.encode_rows(orc.synth_vectors(SEED + 5000 + metric, 0, n, dim), 64)
    Q = orc.synth_vectors(SEED + 5001, 0, 6, dim) * 0.7
    dists = np.stack([orc.all_distances(packed, dim, 64, metric, q) for q in Q])
    radii = np.array([radius_at(d, m) for d, m in zip(dists, (5, 1, 25, 3, 60, 12))])
    want = [orc.search_exact(packed, dim, 64, metric, q, radius=float(r))[:2] for q, r in zip(Q, radii)]
    what = ("radius", MID[metric])
    with open64(dim, metric, sketch_radius=1, radius_mq=0) as ix:
        ix.load(packed)
        rows, dist = ix.search_radius(Q[0], float(radii[0]))
        assert [int(x) for x in rows] == [int(x) for x in want[0][0]] and same(dist, want[0][1]), (what, "lone")
        st = ix.stats()
        assert st["sketch_radius_queries"] + st["sketch_radius_fallbacks"] == 1, (what, st)
        got = ix.search_radius_batch(Q[1:], radii[1:])
        for qi, (g, w) in enumerate(zip(got, want[1:])):
            assert [int(x) for x in g[0]] == [int(x) for x in w[0]], ("rows differ", what, qi)
            assert same(g[1], w[1]), ("distances not bit-equal", what, qi)
        st = ix.stats()
        assert st["sketch_radius_queries"] + st["sketch_radius_fallbacks"] == 6 and st["sketch_radius_queries"] > 0, (what, st)
        recs, _, _ = ix.certificates()
        assert (recs["pass_"] == _lib.SZG_CERT_SKETCH_RADIUS).sum() == st["sketch_radius_queries"], what


@pytest.mark.parametrize("metric", (EUC, COS), ids=["euc", "cos"])
def test_masked_through_the_sketch(metric):
    """One resident mask and 50 tombstones, 17 queries: the matrix sweep's masked forms on the sketch of double rows."""
    dim, n, nq, k = 64, 3000, 17, 10
    packed = orc.encode_rows(orc.synth_vectors(SEED + 5100 + metric, 0, n, dim), 64)
    Q = orc.synth_vectors(SEED + 5101, 0, nq, dim) * 0.7
    allow = np.arange(n) % 5 != 2
    dead = np.random.default_rng(5).permutation(n)[:50]
    eligible = allow.copy()
    eligible[dead] = False
    what = ("masked", MID[metric])
    with open64(dim, metric, sketch_masked=1) as ix:
        ix.load(packed)
        ix.tombstone_rows(dead)
        with ix.mask(allow) as m:
            got = ix.search_topk(Q, k, masks=m)
        assert_answers(got, packed, dim, 64, metric, Q, k, eligible, what)
        st = ix.stats()
        assert st["sketch_queries"] + st["sketch_fallbacks"] == nq and st["sketch_queries"] > 0, (what, st)
        if scan_masked_plan(dim, 8, 16, kp=tss.sketch_kp(k), sketch_masked=1)["serves"]:
            assert ix.sketch_masked_info()["launches"] >= 1, what
