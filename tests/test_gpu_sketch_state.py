"""The sketch index against float64: bytes, bound, keys and lists.

A float32 answer the 8-bit sketch settles is exact only if every link of a chain holds: the build
kernel's bytes and max_ang, the exception list, the sweep's float32 keys of the sketch rows, the lists and merges behind
lb, and D.  The answers never show a broken link -- the candidates are re-ranked on the float32 rows -- so these tests
read the sketch state itself (ScanIndex.sketch_info / sketch_rows) and the certificate trace and hold them against
syzgydb_amd/cert_check.py:

    B    check_sketch_build: every sketch byte, the exception list, max_ang from both sides, the Euclidean scale
    K_s  the sweep's key of a sketch row is within its bound of the float64 key of that sketch row
    L_s  every sketched row outside the lists has a float64 sketch key >= lb      D  D follows from lb
    S    rows outside the candidates are at oracle distance >= D - slack          A  the answers are the oracle's

tests/test_sketch_reference_cpu.py shows without a device that each of these checks can fail.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import ScanIndex, _lib
from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import pack_allow_bits, scan_plan, scan_group_ring_plan
from test_gpu_sketch_lists import crowded_block

pytestmark = pytest.mark.gpu

SEED = 0x53595A4700007000
EUC, COS = 0, 1
METRICS = (EUC, COS)
METRIC_IDS = {EUC: "euc", COS: "cos"}
POOL = ThreadPoolExecutor(8)   # the oracle's C calls release the interpreter lock
MARGINS = cc.Margins()
SHARES = {}                    # (metric, dim) -> the largest share of slack B3 used (scripts/dev_certificates.py prints them)
FLT_MAX = float(np.finfo(np.float32).max)


def sketch_kp(k):
    """Candidates per list of a sketch sweep (SketchCall::run: kk = k + sketch_extra = k + 30; kk + max(16, kk / 2))."""
    kk = k + 30
    return kk + max(16, kk // 2)


def values(packed, dim):
    """The float32 values of packed rows, as float64."""
    return cc.decode_rows(packed, dim, 32)


def open_sketched(dim, metric, devices=None, **options):
    ix = ScanIndex(dim, 32, metric, **({} if devices is None else {"devices": devices}))
    for name, value in dict({"sketch": 1, "sketch_min_rows": 1, "multi_query": 0}, **options).items():
        ix.set_option(name, value)
    ix.trace_certificates(True)
    return ix


def assert_answers(got, packed, dim, metric, Q, k, eligible, what):
    r, d, cnt = got
    allow = None if eligible is None else eligible.astype(np.uint8)
    want = POOL.map(lambda q: orc.search_exact(packed, dim, 32, metric, q, k=k, allow=allow)[:2], Q)
    for qi, (w_rows, w_dist) in enumerate(want):
        assert [int(x) for x in r[qi, : cnt[qi]]] == [int(x) for x in w_rows], ("rows differ", what, qi)
        g = d[qi, : cnt[qi]]
        assert ((g == w_dist) | (np.isnan(g) & np.isnan(w_dist))).all(), ("distances not bit-equal", what, qi)


def searched_state(ix, packed, metric, Q, rebuilt, live, what, k=10):
    """One search, then B on the state it left: the sketch is in sync, one sketch record per query whose slack is the
    state's, the live words are the rows', the answers the oracle's.  -> check_sketch_build's dict"""
    dim = ix.dim
    got = ix.search_topk(Q, k)
    recs, _, dropped = ix.certificates()
    sk = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]
    assert dropped == 0 and sorted(int(x) for x in sk["query"]) == list(range(Q.shape[0])), ("one sketch record per query", what)
    info = ix.sketch_info()
    assert info["exists"] == 1 and info["in_sync"] == 1 and info["disabled"] == 0, (what, info)
    sk_bytes, words = ix.sketch_rows()
    assert sk_bytes.shape == (packed.shape[0], dim), (what, sk_bytes.shape)   # dim bytes per row, no padding
    out = cc.check_sketch_build(values(packed, dim), sk_bytes, info, info["exc_rows"], rebuilt, metric=metric,
                                rec_slack=sk["slack"][0], what=what)
    assert (sk["slack"] == sk["slack"][0]).all()
    want = pack_allow_bits(np.ones(packed.shape[0], dtype=bool) if live is None else live)[0]
    assert (words == want).all(), ("the sketch shards' live words are not the rows'", what, np.flatnonzero(words != want)[:8])
    assert out["share"] <= 1.0
    SHARES[(metric, dim)] = max(SHARES.get((metric, dim), 0.0), out["share"])
    assert_answers(got, packed, dim, metric, Q, k, live, what)
    return out


def test_hooks_refuse_and_never_sync():
    """Both hooks refuse a handle whose rows are not float32; on a float32 handle they report what stands and never
    build or update the sketch: none before the first search, out of sync after a mutation until the next search."""
    from syzgydb_amd import SzgError
    with ScanIndex(16, 8, COS) as ix:
        ix.load(orc.synth_rows(SEED, 0, 100, 16, 8))
        for call in (ix.sketch_info, ix.sketch_rows):
            with pytest.raises(SzgError) as e:
                call()
            assert e.value.code == _lib.SZG_E_INVALID
    packed = orc.synth_rows(SEED + 1, 0, 300, 16, 32)
    with open_sketched(16, COS) as ix:
        ix.load(packed)
        info = ix.sketch_info()
        assert (info["exists"], info["in_sync"], info["rows"], info["n_exc"]) == (0, 0, 0, 0)
        with pytest.raises(SzgError) as e:
            ix.sketch_rows(0, 1)
        assert e.value.code == _lib.SZG_E_RANGE
        Q = orc.synth_vectors(SEED + 2, 0, 2, 16)
        searched_state(ix, packed, COS, Q, True, None, ("hooks",))
        ix.overwrite(3, packed[4])
        info = ix.sketch_info()
        assert (info["exists"], info["in_sync"], info["rows"]) == (1, 0, 300)
        assert (ix.sketch_rows(3, 1)[0] != ix.sketch_rows(4, 1)[0]).any()   # (the stale sketch row: still row 3's own)
        with pytest.raises(SzgError) as e:
            ix.sketch_rows(299, 2)
        assert e.value.code == _lib.SZG_E_RANGE
        assert ix.sketch_info()["in_sync"] == 0


# ---- the build kernel ---------------------------------------------------------------------------------------------------

BUILD_DIMS = (1, 3, 15, 16, 17, 63, 64, 65, 100, 768, 1024, 1025, 1040, 2049)
BUILD_ROWS = 1501   # not a multiple of the 4 waves (rows) of a block
BAD_AT = {"inf first": 17, "nan last": 18, "-inf middle": 19, "nan first": 20, "inf last": 21, "nan middle": 22}


def build_rows(dim, metric):
    """orc.synth_vectors times per-row factors -- 1e-30 .. 1e30 under cosine (each row has its own scale), 1e-3 .. 1e3
    under Euclid (one scale: wider, and most rows would have no bytes to compare) -- and hand-made rows 10 .. 22."""
    n = BUILD_ROWS
    rng = np.random.default_rng(dim * 2 + metric)
    span = 30.0 if metric == COS else 3.0
    vec = orc.synth_vectors(SEED + dim, 0, n, dim) * 10.0 ** rng.permutation(np.linspace(-span, span, n))[:, None]
    alt = np.where(np.arange(dim) % 3 == 0, -1.0, 1.0)
    vec[10] = 0.0
    vec[10, dim - 1] = -2.5                        # one non-zero element
    vec[11] = 0.75 * alt                           # every |x_i| equal: the sketch is exact, the angle 0
    vec[12] = 0.0 * alt                            # +-0.0: no direction
    vec[13, ::2] = -0.0                            # -0.0 among ordinary elements
    if metric == COS:
        vec[14, dim // 2] = FLT_MAX                # (Euclid: appended later -- it becomes the scale of every row)
    vec[15] = alt * 1.4e-45 * (1 + np.arange(dim) % 3)   # denormals only
    vec[16] = 0.0
    mid = dim // 2
    for name, r in BAD_AT.items():
        at = {"first": 0, "last": dim - 1, "middle": mid}[name.split()[1]]
        vec[r, at] = {"inf": np.inf, "-inf": -np.inf, "nan": np.nan}[name.split()[0]]
    return vec


@pytest.mark.parametrize("metric", METRICS, ids=["euc", "cos"])
@pytest.mark.parametrize("dim", BUILD_DIMS)
def test_build_kernel(dim, metric):
    """B after one search of 2 queries: a lone short piece (1, 3, 15), whole and ragged pieces (16, 17, 63 .. 65, 100),
    768, every lane one piece (1024), a second piece on lane 0 (1025, 1040) and on every lane (2049)."""
    vec = build_rows(dim, metric)
    packed = orc.encode_rows(vec, 32)
    Q = orc.synth_vectors(SEED + dim + 1, 0, 2, dim)
    what = ("build", dim, METRIC_IDS[metric])
    with open_sketched(dim, metric) as ix:
        ix.load(packed)
        assert ix.sketch_info()["exists"] == 0
        out = searched_state(ix, packed, metric, Q, True, None, what)
        exc = set(int(r) for r in ix.sketch_info()["exc_rows"])
        bad = set(BAD_AT.values())
        zero = {12, 16} | ({13} if dim == 1 else set())   # (one dimension: row 13 is -0.0 and nothing else)
        assert exc == (bad | zero if metric == COS else bad), (what, sorted(exc))   # the zero rows: cosine only
        assert out["sketched"] == BUILD_ROWS - len(exc)
        if metric == EUC:   # the largest finite float32 becomes the one scale: a rebuild, and an ordinary row
            top = np.zeros((1, dim))
            top[0, dim // 2] = -FLT_MAX
            packed = np.concatenate([packed, orc.encode_rows(top, 32)])
            ix.append(packed[-1:])
            assert ix.sketch_info()["in_sync"] == 0
            searched_state(ix, packed, metric, Q, True, None, what + ("largest float",))
            info = ix.sketch_info()
            assert info["gscale"] == FLT_MAX and set(int(r) for r in info["exc_rows"]) == bad, (what, info)


# ---- the state through mutations ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", (None, [0, 0]), ids=["1shard", "2shards"])
@pytest.mark.parametrize("metric", METRICS, ids=["euc", "cos"])
@pytest.mark.parametrize("dim", (96, 1040))
def test_state_sequence(dim, metric, devices):
    """B, the live words and the "in sync" flag after a search following each mutation."""
    n0, n_app = 5300, 700
    rng = np.random.default_rng(dim + metric)
    pool = orc.encode_rows(orc.synth_vectors(SEED + 100 + dim, 0, n0 + n_app + 5300 + 1500, dim), 32)
    fresh = pool[n0 + n_app:]
    Q = orc.synth_vectors(SEED + 101 + dim, 0, 2, dim) * 0.7
    what = ("sequence", dim, METRIC_IDS[metric], "shards", 1 if devices is None else 2)
    zero = orc.encode_rows(np.zeros((1, dim)), 32)
    is_cos = metric == COS

    def step(name, rebuilt, live=None):
        return searched_state(ix, packed, metric, Q, rebuilt, live, what + (name,))

    with open_sketched(dim, metric, devices) as ix:
        packed = pool[:n0].copy()
        if is_cos:
            packed[7] = zero[0]
        ix.load(packed)
        step("load", True)
        # 1. appended rows: only they are built
        packed = np.concatenate([packed, pool[n0:n0 + n_app]])
        ix.append(packed[n0:])
        assert ix.sketch_info()["in_sync"] == 0
        before = step("append", False)

        def far_row():
            """a row farther from its sketch than any so far: every element half a step from its byte's value, but
            one.  max_ang must follow the reference's maximum up."""
            scale = ix.sketch_info()["gscale"] or 1.0
            far = np.full((1, dim), 1e-6 * scale)
            far[0, 0] = 0.9 * scale
            packed[n0 + 3] = orc.encode_rows(far, 32)[0]
            ix.overwrite(n0 + 3, packed[n0 + 3])
            risen = step("overwrite far", False)
            assert risen["largest"] > 1.2 * before["largest"] > 0, (what, risen, before)
            assert ix.sketch_info()["max_ang"] >= risen["largest"] - risen["allowance"] > before["largest"]

        # 2. single overwrites: good -> zero, zero -> good, and the far row
        if is_cos:
            packed[5] = zero[0]
            ix.overwrite(5, packed[5])
            packed[7] = fresh[0]
            ix.overwrite(7, packed[7])
            step("overwrite zero/good", False)
            assert set(int(r) for r in ix.sketch_info()["exc_rows"]) == {5, 7}, what   # (7 stays listed until a rebuild)
            far_row()
        else:   # (a Euclidean zero row is sketched, and as far from its sketch as a row can be: the far row comes first)
            far_row()
            packed[5] = zero[0]
            ix.overwrite(5, packed[5])
            step("overwrite good by zero", False)
            packed[5] = fresh[0]
            ix.overwrite(5, packed[5])
            step("overwrite zero by good", False)
            assert len(ix.sketch_info()["exc_rows"]) == 0, what
        # 3. 300 listed rows: one launch over the list
        at = rng.permutation(n0 + n_app)[:300]
        packed[at] = fresh[1:301]
        ix.overwrite_rows(at, packed[at])
        step("overwrite_rows 300", False)
        # 4. 5 000 rows: more than the list takes -- a full rebuild
        at = rng.permutation(n0 + n_app)[:5000]
        packed[at] = fresh[301:5301]
        ix.overwrite_rows(at, packed[at])
        step("overwrite_rows 5000", True)
        assert len(ix.sketch_info()["exc_rows"]) == (1 if is_cos and 5 not in set(int(x) for x in at) else 0)
        if not is_cos:
            # 5. a row at twice the scale: a rebuild, the scale doubles; then a row overwritten to four times: no
            # rebuild, it becomes an exception
            g = ix.sketch_info()["gscale"]
            big = values(fresh[5301:5302], dim)
            big[0, dim - 1] = 2.0 * g
            packed = np.concatenate([packed, orc.encode_rows(big, 32)])
            ix.append(packed[-1:])
            step("append 2x scale", True)
            assert ix.sketch_info()["gscale"] == 2.0 * g
            big[0, 1] = -8.0 * g
            packed[40] = orc.encode_rows(big, 32)[0]
            ix.overwrite(40, packed[40])
            step("overwrite 4x scale", False)
            info = ix.sketch_info()
            assert info["gscale"] == 2.0 * g and [int(r) for r in info["exc_rows"]] == [40], (what, info)
        # 6. tombstones
        n = packed.shape[0]
        live = np.ones(n, dtype=bool)
        dead = np.concatenate([np.arange(3, n, 7), [n - 1, 64, 65]])
        live[dead] = False
        ix.tombstone_rows(dead)
        assert ix.sketch_info()["in_sync"] == 0
        step("tombstones", False, live)
        # 7. compaction, then a shuffled order: rebuilt, the bytes follow the rows
        ix.compact()
        packed = packed[live]
        step("compact", True)
        perm = rng.permutation(packed.shape[0])
        ix.reorder(perm)
        packed = packed[perm]
        step("reorder", True)
        # 8. a second load
        packed = fresh[3000:4500].copy()
        ix.load(packed)
        step("second load", True)
        # more rows without a usable sketch than the list holds: the sketch index is given back, the answers stay
        void = np.zeros((4200, dim)) if is_cos else np.full((4200, dim), np.nan)
        packed = np.concatenate([packed, orc.encode_rows(void, 32)])
        ix.append(packed[1500:])
        got = ix.search_topk(Q, 10)
        info = ix.sketch_info()
        assert info["disabled"] == 1 and info["exists"] == 0 and info["in_sync"] == 0, (what, info)
        assert_answers(got, packed, dim, metric, Q, 10, None, what + ("disabled",))


# ---- keys and lists ---------------------------------------------------------------------------------------------------------

def rows_per_step(dim, kp):
    p = scan_plan(dim, 8, 1 << 22, kp=kp)
    return p["grid"] * (p["block"] // 64) * 16 if p["tiled"] else p["grid"] * (p["block"] // 64) * p["gpw"]


def ring_depths():
    return scan_group_ring_plan(768, 8, 16, kp=sketch_kp(10), scan_group=4)["depths"]


@functools.lru_cache(maxsize=1)
def synth_corpus(seed, n, dim):
    cuts = np.linspace(0, n, 9).astype(np.int64)
    parts = POOL.map(lambda i: orc.synth_rows(seed, int(cuts[i]), int(cuts[i + 1] - cuts[i]), dim, 32), range(8))
    return np.concatenate(list(parts))


def traced_sketch(ix, corpus, Q, k, what, eligible=None, **filt):
    """One top-k call through the sketch: K_s, L_s, D and S on its sketch records (K, L, C on those of the queries it
    handed over), A on the answers.  -> (keys checked, queries settled)"""
    Q = np.atleast_2d(Q)
    got = ix.search_topk(Q, k, **filt)
    recs, ents, dropped = ix.certificates()
    sk = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]
    assert sorted(int(x) for x in sk["query"]) == list(range(Q.shape[0])), ("one sketch record per query", what)
    info = ix.sketch_info()
    assert info["in_sync"] == 1, (what, info)
    sk_corpus = cc.Corpus(ix.sketch_rows()[0], corpus.dim, 8, corpus.metric)
    dists = np.stack(list(POOL.map(lambda q: orc.all_distances(corpus.packed, corpus.dim, 32, corpus.metric, q), Q)))
    s = cc.check(corpus, Q, recs, ents, dropped, eligible=eligible, dists=dists, margins=MARGINS, what=what,
                 sketch=(sk_corpus, info["gscale"], info["exc_rows"]))
    assert s.skipped == 0, ("candidates without a bound on a corpus that plants no bad row", what, sorted(s.skipped_rows)[:8])
    assert s.checked > 0, ("no key was checked", what)
    assert_answers(got, corpus.packed, corpus.dim, corpus.metric, Q, k, eligible, what)
    return s.checked, int((sk["certified"] == 1).sum())


# (dim, s, r, queries, scan_group, sketch_planes, sketch_list: 0 automatic / -1 kp / 96, k, metric, multi_query, ring)
# -- corners of the lattice: every value of every axis, and the pairs that share code (groups x planes x list form)
KEY_CASES = [
    (96, 1, 0, 1, 1, 0, 0, 10, COS, 0, 0), (96, 3, 77, 17, 4, 3, -1, 1, EUC, 0, 0),
    (96, 1, 77, 3, 4, 0, 96, 34, EUC, 0, 0), (96, 1, 0, 1, 1, 3, 0, 10, EUC, 1, 0),
    (100, 1, 77, 16, 4, 0, 0, 10, EUC, 0, 0), (100, 3, 0, 3, 1, 3, 96, 1, COS, 0, 0),
    (100, 1, 0, 17, 4, 3, -1, 34, COS, 0, 0), (100, 1, 77, 1, 4, 0, 0, 34, COS, 1, 0),
    (384, 1, 77, 16, 4, 0, 0, 10, COS, 0, 0), (384, 3, 0, 17, 1, 3, -1, 34, EUC, 0, 0),
    (384, 1, 0, 3, 4, 3, 96, 1, EUC, 0, 0), (384, 1, 77, 1, 1, 0, 0, 1, COS, 1, 0),
    (768, 1, 0, 16, 4, 0, 0, 10, EUC, 0, 0), (768, 1, 77, 17, 4, 0, 0, 10, COS, 0, 1),
    (768, 3, 77, 16, 4, 3, -1, 10, COS, 0, 2), (768, 1, 0, 3, 4, 0, 96, 34, EUC, 0, 2),
    (768, 1, 77, 17, 1, 3, 0, 1, EUC, 0, 0), (768, 1, 0, 16, 4, 3, 96, 10, COS, 0, 1),
]


def key_case_id(c):
    dim, s, r, nq, group, planes, lst, k, metric, mq, ring = c
    return "d%d-s%d-r%d-q%d-g%d-p%d-l%d-k%d-%s-mq%d-ring%d" % (dim, s, r, nq, group, planes, lst, k, METRIC_IDS[metric], mq, ring)


@pytest.mark.parametrize("case", KEY_CASES, ids=[key_case_id(c) for c in KEY_CASES])
def test_keys_and_lists(case):
    """K_s, L_s, D, S and A: any-shape lane maps (96, 100) and the row-shape kernels (384, 768; ring: 0 automatic, 1 and
    2 the first and last depth scan_group_ring_plan reports), s whole steps of the sketch sweep's launch plus r rows, then
    the same under a mask without every fifth row and with tombstones."""
    dim, s, r, nq, group, planes, lst, k, metric, mq, ring = case
    kp = sketch_kp(k)
    n = s * rows_per_step(dim, kp) + r
    seed = SEED + 7000 + dim * 100 + s * 10 + (r % 7) + k
    corpus = cc.Corpus(synth_corpus(seed, n, dim), dim, 32, metric)
    Q = orc.synth_vectors(seed + 1, 0, nq, dim) * 0.7
    depth = 0 if ring == 0 else ring_depths()[0 if ring == 1 else -1]
    what = ("keys", key_case_id(case), "rows", n)
    with open_sketched(dim, metric, multi_query=mq, scan_group=group, sketch_planes=planes, scan_group_ring=depth,
                       sketch_list={0: 0, -1: kp, 96: 96}[lst]) as ix:
        ix.synth(n, seed)
        assert (ix.read_rows(n - 1, 1) == corpus.packed[n - 1:]).all()   # device synthesis == the oracle's
        checked, settled = traced_sketch(ix, corpus, Q, k, what)
        allow = np.arange(n) % 5 != 2
        c2, s2 = traced_sketch(ix, corpus, Q, k, what + ("mask",), eligible=allow, allow=np.stack([allow] * nq))
        dead = np.arange(n) % 9 == 4
        ix.tombstone_rows(np.flatnonzero(dead))
        c3, s3 = traced_sketch(ix, corpus, Q, k, what + ("tombstones",), eligible=~dead)
        assert settled + s2 + s3 > 0, ("the sketch settled no query: S and D never ran", what)
        st = ix.stats()
        assert st["sketch_queries"] == settled + s2 + s3 and st["mq_queries"] == 0, (what, st)


def test_drop_bound_sets_lb():
    """40 of a query's best rows in one block, short lists: the drop bound, not the kp-th key, is lb -- and L_s holds
    against it (the queries take the full sweep; with the full lists they settle)."""
    dim, k = 48, 10
    V, q = crowded_block(1400, dim)
    corpus = cc.Corpus(orc.encode_rows(V, 32), dim, 32, COS)
    Q = np.stack([q, q * 2.0, q + 1e-4 * np.arange(dim) / dim])
    with open_sketched(dim, COS) as ix:
        ix.load(corpus.packed)
        lb = {}
        for lst in (0, 4096):
            ix.set_option("sketch_list", lst)
            ix.search_topk(Q, k)
            recs, ents, _ = ix.certificates()
            sk = recs[recs["pass_"] == _lib.SZG_CERT_SKETCH]
            lb[lst] = sk["thr_min"][np.argsort(sk["query"])]
            ix.reset_stats()
            checked, settled = traced_sketch(ix, corpus, Q, k, ("drop bound", "sketch_list", lst))
            assert settled == (0 if lst == 0 else 3), (lst, settled)
        assert (lb[0] < lb[4096]).all(), ("the drop bound did not lower lb", lb)


def test_margins_and_shares():
    """What the tests above measured: every K_s ratio and every share of slack is at most 1 (asserted where measured;
    scripts/dev_certificates.py writes the figures to profiles/certificate_margins.txt)."""
    for what, ratio in MARGINS.worst.items():
        assert ratio <= 1.0, (what, ratio)
    for what, share in SHARES.items():
        assert share <= 1.0, (what, share)
    for line in MARGINS.lines() + ["B3 slack left  %s dim %4d  %.3e" % (METRIC_IDS[m], d, 1.0 - v) for (m, d), v in sorted(SHARES.items())]:
        print(line)
