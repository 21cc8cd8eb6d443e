"""Resident metadata columns (szg_column / ScanColumn): a comparison against a constant writes the words of a filter
mask on the card.  The words and counts are checked against numpy at every size where the layout changes (the tail of
a word, the padding word of a pair, an odd word count, parts that start at a shard boundary); the masks are then used
like any others; the Collection answers Search(Where=) exactly as it answers Search(Filter=) with the host evaluator of
the same expression."""
import operator

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import (Collection, CollectionOptions, Field, ScanIndex, SearchArgs, SzgError, SZG_COSINE, _lib,
                         pack_allow_bits)
from test_columns_cpu import TRUTH

pytestmark = pytest.mark.gpu

SEED = 0x53595A4700000000
DIM, BITS = 8, 8
SIZES = [1, 63, 64, 65, 127, 128, 129, 777, 1000]
OPS = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}


def packed(b):
    return pack_allow_bits(np.asarray(b, dtype=bool))[0]


def check_mask(m, want, what=""):
    """read() equals the packed verdicts (so the tail bits are 0) and count equals the popcount."""
    words = m.read()
    assert (words == packed(want)).all(), what
    assert m.count == int(np.asarray(want).sum()), what
    n = len(want)
    if n % 64:
        assert int(words[-1]) >> (n % 64) == 0, what
    m.close()


def f64_values(n, seed):
    """Finite values with duplicates, and -0.0, 0.0, inf, -inf and NaN where there is room."""
    rng = np.random.default_rng(seed)
    v = np.round(rng.normal(0, 10, n), 1)
    for i, special in zip(rng.permutation(n)[:10], [-0.0, 0.0, np.inf, -np.inf, np.nan, np.nan, 0.0, -0.0, 5.0, 5.0]):
        v[i] = special
    return v


def present_variants(n, seed):
    """(name, what is passed as present=, the bool it means)"""
    rng = np.random.default_rng(seed)
    rnd = rng.random(n) < 0.7
    ones = np.full((n + 63) // 64, np.uint64(0xFFFFFFFFFFFFFFFF))   # every bit set, the tail bits included
    return [("none", None, np.ones(n, bool)), ("random", rnd, rnd), ("zero", np.zeros(n, bool), np.zeros(n, bool)),
            ("ones+tail", ones, np.ones(n, bool))]


def loaded_index(n, devices, bits=BITS, dim=DIM):
    ix = ScanIndex(dim, bits, SZG_COSINE, devices=devices)
    ix.load(orc.synth_rows(SEED, 0, n, dim, bits))
    return ix


# ---- 1. words and counts against numpy ------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("n", SIZES)
def test_f64_words_and_counts(n, devices):
    v = f64_values(n, n)
    finite = v[np.isfinite(v)]
    stored = float(finite[len(finite) // 2]) if finite.size else 1.0
    constants = [-1e300, 1e300, stored, 0.0, np.inf]   # below / above every finite value, a stored one, +-0, inf
    with loaded_index(n, devices) as ix, np.errstate(invalid="ignore"):
        base_bool = np.random.default_rng(n + 7).random(n) < 0.6
        base = ix.mask(base_bool)
        for pname, parg, pres in present_variants(n, n + 1):
            with ix.column(v, present=parg) as col:
                assert col.rows == n and col.kind == _lib.SZG_COL_F64
                got_v, got_p = col.read()
                assert (got_v.view(np.uint64) == v.view(np.uint64)).all() and (got_p == pres).all()
                for bm, bb in ((None, np.ones(n, bool)), (base, base_bool)):
                    for op, fn in OPS.items():
                        for c in constants:
                            check_mask(col.where(op, c, base=bm), fn(v, c) & pres & bb, (pname, op, c, bm is not None))
                    check_mask(col.present(base=bm), pres & bb, pname)
                    # IN-lists: 0, 1, 3 and 1024 constants with duplicates, NaN among them (it equals nothing)
                    for lst in ([], [stored], [stored, 0.0, np.nan], list(np.resize(np.unique(finite)[:700], 1024))):
                        want = np.isin(v, [x for x in lst if x == x]) & pres & bb
                        check_mask(col.isin(lst, base=bm), want, (pname, "in", len(lst)))
                check_mask(col < stored, (v < stored) & pres)
                check_mask(col >= stored, (v >= stored) & pres)
                check_mask(col.eq(stored), (v == stored) & pres)
                check_mask(col.ne(stored), (v != stored) & pres)
                with pytest.raises(SzgError) as e:
                    col.isin(np.arange(1025.0))
                assert e.value.code == _lib.SZG_E_UNSUPPORTED
                with pytest.raises(SzgError) as e:
                    col.where(9, 1.0)
                assert e.value.code == _lib.SZG_E_INVALID
                with pytest.raises(SzgError) as e:   # a kind that does not match the call
                    col.codes([True])
                assert e.value.code == _lib.SZG_E_INVALID


@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("n", SIZES)
def test_u32_words_and_counts(n, devices):
    rng = np.random.default_rng(n + 100)
    codes = rng.integers(0, 200, n).astype(np.uint32)
    codes[rng.integers(0, n)] = 0xFFFFFFFF   # far beyond every bitmap
    with loaded_index(n, devices) as ix:
        base_bool = rng.random(n) < 0.6
        base = ix.mask(base_bool)
        for pname, parg, pres in present_variants(n, n + 2):
            with ix.column(codes, present=parg) as col:
                assert col.kind == _lib.SZG_COL_U32
                got_v, got_p = col.read()
                assert (got_v == codes).all() and (got_p == pres).all()
                for bm, bb in ((None, np.ones(n, bool)), (base, base_bool)):
                    # n_codes below the largest stored code, at and around a word of the bitmap, none at all
                    for n_codes in (0, 1, 12, 64, 65, 130, 200):
                        allowed = rng.random(n_codes) < 0.5
                        lut = np.zeros(1 << 8, bool)
                        lut[:n_codes] = allowed
                        want = np.where(codes < n_codes, lut[np.minimum(codes, 255)], False) & pres & bb
                        check_mask(col.codes(allowed, base=bm), want, (pname, n_codes, bm is not None))
                    check_mask(col.codes(np.ones(200, bool), base=bm), (codes < 200) & pres & bb, pname)
                    check_mask(col.present(base=bm), pres & bb, pname)
                with pytest.raises(SzgError) as e:
                    col.where("<", 1.0)
                assert e.value.code == _lib.SZG_E_INVALID


# ---- 2. a `where` mask is a mask ---------------------------------------------------------------------------------------

def check_search(ix, rows, dim, bits, Q, k, allowed, mask, radius=None):
    """masks= equals allow= of the same words bit for bit, and the oracle."""
    Q = np.atleast_2d(Q)
    A = np.repeat(allowed[None, :], Q.shape[0], axis=0)
    r, d, c = ix.search_topk(Q, k, masks=mask)
    r2, d2, c2 = ix.search_topk(Q, k, allow=A)
    assert (c == c2).all() and (r == r2).all() and (d.view(np.uint64) == d2.view(np.uint64)).all()
    for i in range(Q.shape[0]):
        o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, SZG_COSINE, Q[i], k=k, allow=allowed.astype(np.uint8))
        assert list(map(int, r[i, : c[i]])) == list(map(int, o_rows))
        assert (d[i, : c[i]].view(np.uint64) == np.asarray(o_dist, dtype=np.float64).view(np.uint64)).all()
    if radius is not None:
        hits = ix.search_radius_batch(Q, radius, masks=mask)
        hits2 = ix.search_radius_batch(Q, radius, allow=A)
        for i in range(Q.shape[0]):
            assert (hits[i][0] == hits2[i][0]).all() and (hits[i][1].view(np.uint64) == hits2[i][1].view(np.uint64)).all()
            o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, SZG_COSINE, Q[i], radius=radius,
                                                 allow=allowed.astype(np.uint8))
            assert list(map(int, hits[i][0])) == list(map(int, o_rows))
            assert (hits[i][1].view(np.uint64) == np.asarray(o_dist, dtype=np.float64).view(np.uint64)).all()


def test_where_mask_algebra_and_compaction():
    n = 1000
    v = f64_values(n, 3)
    other_bool = np.random.default_rng(4).random(n) < 0.5
    with loaded_index(n, [0, 0]) as ix, np.errstate(invalid="ignore"):
        col = ix.column(v)
        other = ix.mask(other_bool)
        both = (col < 2.5) & other
        assert (both.read() == packed((v < 2.5) & other_bool)).all() and both.count == int(((v < 2.5) & other_bool).sum())
        check_mask(~(col < 2.5), ~(v < 2.5))
        check_mask((col >= 0.0) | other, (v >= 0.0) | other_bool)
        live0 = ix.mask_stats()["live_masks"]
        m = col < 2.5
        assert ix.mask_stats()["live_masks"] == live0 + 1   # accounted like every mask
        # a compaction without tombstones moves nothing: column and masks stay valid
        ix.compact(carry=[m])
        check_mask(col.where("<", 2.5, base=both), (v < 2.5) & other_bool)
        # with tombstones the carried mask is renumbered like any other mask
        dead = [0, 63, 64, 500, n - 1]
        for r in dead:
            ix.tombstone(r)
        check_mask(col > 0.0, v > 0.0)   # tombstones leave a column valid
        new_of_old = ix.compact(carry=[m])
        keep = np.flatnonzero(new_of_old != np.uint64(0xFFFFFFFFFFFFFFFF))
        assert ix.rows == n - len(dead)
        assert (m.read() == packed((v < 2.5)[keep])).all() and m.count == int((v < 2.5)[keep].sum())


def test_one_sweep_search_with_where_mask():
    n, k = 777, 10
    rows = orc.synth_rows(SEED, 0, n, DIM, BITS)
    v = f64_values(n, 5)
    with loaded_index(n, None) as ix, np.errstate(invalid="ignore"):
        ix.set_option("multi_query", 0)
        col = ix.column(v, present=np.random.default_rng(6).random(n) < 0.8)
        _, pres = col.read()
        m = col <= 1.0
        Q = orc.synth_vectors(SEED + 1, 0, 2, DIM)
        check_search(ix, rows, DIM, BITS, Q[0], k, (v <= 1.0) & pres, m, radius=0.6)
        check_search(ix, rows, DIM, BITS, Q, 1, (v <= 1.0) & pres, m)
        assert ix.stats()["mq_queries"] == 0


def test_shared_sweep_search_with_where_mask():
    n, k = 1000, 10
    rows = orc.synth_rows(SEED, 0, n, DIM, BITS)
    codes = np.random.default_rng(8).integers(0, 9, n).astype(np.uint32)
    allowed_codes = np.array([1, 0, 0, 1, 1, 0, 1, 0, 0], dtype=bool)
    with loaded_index(n, [0, 0]) as ix:
        col = ix.column(codes)
        m = col.codes(allowed_codes)
        Q = orc.synth_vectors(SEED + 2, 0, 3, DIM)
        ix.reset_stats()
        check_search(ix, rows, DIM, BITS, Q, k, allowed_codes[codes], m, radius=0.6)
        assert ix.stats()["mq_queries"] >= 3


def test_sketch_prepass_search_with_where_mask():
    n, k, bits = 4096, 5, 32
    rows = orc.synth_rows(SEED, 0, n, DIM, bits)
    v = f64_values(n, 9)
    with loaded_index(n, None, bits=bits) as ix, np.errstate(invalid="ignore"):
        ix.set_option("sketch", 1)
        col = ix.column(v)
        m = col.where(">", -3.0)
        Q = orc.synth_vectors(SEED + 3, 0, 2, DIM)
        ix.reset_stats()
        for i in range(2):
            check_search(ix, rows, DIM, bits, Q[i], k, v > -3.0, m)
        assert ix.stats()["sketch_queries"] >= 1


# ---- 3. append and set --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f64", "u32"])
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_append_and_set(devices, kind):
    rng = np.random.default_rng(11)
    total = 100 + 37 + 200
    all_rows = orc.synth_rows(SEED, 0, total, DIM, BITS)
    if kind == "f64":
        v = f64_values(total, 12)
        new_values = [123.5, -7.25, np.nan]
    else:
        v = rng.integers(0, 50, total).astype(np.uint32)
        new_values = [3, 49, 7]
    pres = rng.random(total) < 0.7

    def verify(col, n):
        got_v, got_p = col.read()
        assert col.rows == n and got_v.size == n
        same = (got_v.view(np.uint64) == v[:n].view(np.uint64)) if kind == "f64" else (got_v == v[:n])
        assert (same | ~pres[:n]).all() and (got_p == pres[:n]).all()   # (an absent row's stored value is not defined)
        with np.errstate(invalid="ignore"):
            if kind == "f64":
                check_mask(col < 1.0, (v[:n] < 1.0) & pres[:n])
                check_mask(col.ne(5.0), (v[:n] != 5.0) & pres[:n])
            else:
                allowed = np.arange(50) % 3 == 0
                check_mask(col.codes(allowed), allowed[v[:n]] & pres[:n])
        check_mask(col.present(), pres[:n])

    with ScanIndex(DIM, BITS, SZG_COSINE, devices=devices) as ix:
        ix.load(all_rows[:100])
        col = ix.column(v[:100], present=pres[:100])
        verify(col, 100)
        # 37 rows to the index, then to the column: its present bits are relative to the block (an unaligned shift)
        ix.append(all_rows[100:137])
        with pytest.raises(SzgError) as e:
            col.present()
        assert e.value.code == _lib.SZG_E_INVALID and "short column" in str(e.value)
        col.append(v[100:137], present=pres[100:137])
        verify(col, 137)
        # 200 more: across words and pairs (and a shard's growth)
        ix.append(all_rows[137:])
        col.append(v[137:], present=packed(pres[137:]))   # (words this time)
        verify(col, total)
        with pytest.raises(SzgError) as e:
            col.append(v[:1])
        assert e.value.code == _lib.SZG_E_RANGE
        verify(col, total)   # an error leaves the column as it was
        # single rows: the first, the last, one at a word boundary -- a value, then absent
        for row, value in zip((0, total - 1, 64), new_values):
            col.set(row, value)
            v[row], pres[row] = value, True
            verify(col, total)
        for row in (0, total - 1, 64, 63):
            col.set(row, None)
            pres[row] = False
            verify(col, total)
        with pytest.raises(SzgError) as e:
            col.set(total, new_values[0])
        assert e.value.code == _lib.SZG_E_RANGE
        # all present by default on append as well
        ix.append(all_rows[:3])
        col.append(v[:3])
        v, pres = np.concatenate([v, v[:3]]), np.concatenate([pres, np.ones(3, bool)])
        verify(col, total + 3)


def test_column_shorter_than_the_index_at_creation():
    n = 300
    v = f64_values(n, 13)
    with loaded_index(n, [0, 0]) as ix, np.errstate(invalid="ignore"):
        col = ix.column(v[:130])
        assert col.rows == 130
        with pytest.raises(SzgError) as e:
            col < 1.0
        assert "short column" in str(e.value)
        col.append(v[130:])
        check_mask(col < 1.0, v < 1.0)
        with pytest.raises(SzgError) as e:
            ix.column(np.zeros(n + 1))
        assert e.value.code == _lib.SZG_E_RANGE


# ---- 4. staleness ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["load", "synth", "reorder", "compact"])
def test_stale_column(how):
    n = 200
    v = f64_values(n, 14)
    with loaded_index(n, [0, 0]) as ix:
        col = ix.column(v, present=np.arange(n) % 2 == 0)
        if how == "load":
            ix.load(orc.synth_rows(SEED + 1, 0, n, DIM, BITS))
        elif how == "synth":
            ix.synth(n, 5)
        elif how == "reorder":
            ix.reorder(np.arange(n)[::-1])
        else:
            ix.tombstone(7)
            ix.compact()
        for call in (lambda: col < 1.0, lambda: col.isin([1.0]), lambda: col.present(), lambda: col.append([1.0]),
                     lambda: col.set(0, 1.0)):
            with pytest.raises(SzgError) as e:
                call()
            assert e.value.code == _lib.SZG_E_INVALID and "stale column" in str(e.value)
        assert col.rows == n
        got_v, got_p = col.read()
        assert (got_v.view(np.uint64) == v.view(np.uint64)).all() and (got_p == (np.arange(n) % 2 == 0)).all()
        col.close()


def test_base_mask_checks_and_clean_close():
    n = 200
    v = f64_values(n, 15)
    ix = loaded_index(n, None)
    other = loaded_index(n, None)
    col = ix.column(v)
    foreign = other.mask(np.ones(n, bool))
    with pytest.raises(SzgError) as e:
        col.where("<", 1.0, base=foreign)
    assert e.value.code == _lib.SZG_E_INVALID
    old = ix.mask(np.ones(n, bool))
    ix.append(orc.synth_rows(SEED + 2, 0, 1, DIM, BITS))   # `old` is stale now, the column short
    col.append([2.0])
    with pytest.raises(SzgError) as e:
        col.where("<", 1.0, base=old)
    assert e.value.code == _lib.SZG_E_INVALID and "stale mask" in str(e.value)
    with np.errstate(invalid="ignore"):
        check_mask(col < 1.0, np.append(v, 2.0) < 1.0)
    # no tombstones: a compaction leaves the column valid
    ix.compact()
    check_mask(col.present(), np.ones(n + 1, bool))
    col2 = ix.column(np.arange(n + 1, dtype=np.uint32))
    other.close()
    ix.close()   # with live columns and masks: they are closed first
    assert not col._h and not col2._h


# ---- 5. the Collection ------------------------------------------------------------------------------------------------

price, name, flag = Field("price"), Field("name"), Field("flag")

EXPRESSIONS = [
    price == 5, price != 5, price < 5, price <= 4.5, price > 5, price >= 1000, price == 0,
    name == "abc", name != "abc", name < "b", name >= "b", name > "z", name < "é",
    price.isin([1, 5, 9]), price.notin([1, 5]), name.isin(["a", "b", "abc"]), name.notin(["abc"]),
    name.startswith("ab"), name.endswith("bc"), name.contains("b"),
    (price == 5) | (name < "b"), (name < "b") | (price == 5), (price < 5) & (name == "a"),
    ~(price < 5), ~(price == 5), ~(~(name.startswith("a"))), (price != 5) | ~(name.contains("a")),
    ((price < 5) | name.isin(["a", "zz"])) & ~name.endswith("q"),
]
FALLBACKS = [flag == 1, (price < 5) | (flag != 1), price == "5", name < 5, price.isin([1, "5"])]


def collection_metadata(n):
    pool = sorted({meta for _, meta, _, _ in TRUTH})   # every row of the CPU truth table
    rng = np.random.default_rng(21)
    names = ["a", "ab", "abc", "abd", "b", "zz", "é", "q", ""]
    out = []
    for i in range(n):
        if i < len(pool):
            out.append(pool[i])
        else:
            out.append(('{"price": %s, "name": "%s", "flag": %s}'
                        % (rng.integers(0, 12) * 0.5, names[rng.integers(len(names))], "true" if i % 2 else "false")).encode())
    return out


def assert_same_answers(c, q, exprs, k=10):
    def as_filter(e):
        return lambda id_, meta: e.evaluate(meta)

    for e in exprs:
        got = c.Search(SearchArgs(Vector=q[0], K=k, Where=e))
        want = c.Search(SearchArgs(Vector=q[0], K=k, Filter=as_filter(e)))
        assert [r.ID for r in got.Results] == [r.ID for r in want.Results], e.text()
        assert [r.Distance for r in got.Results] == [r.Distance for r in want.Results], e.text()
        assert got.PercentSearched == want.PercentSearched
    got = c.SearchBatch([SearchArgs(Vector=q[i % len(q)], K=k, Where=e) for i, e in enumerate(exprs)])
    want = c.SearchBatch([SearchArgs(Vector=q[i % len(q)], K=k, Filter=as_filter(e)) for i, e in enumerate(exprs)])
    for e, g, w in zip(exprs, got, want):
        assert [(r.ID, r.Distance) for r in g.Results] == [(r.ID, r.Distance) for r in w.Results], e.text()
    # radius and listing mode go the same way
    e = exprs[0]
    got = c.Search(SearchArgs(Vector=q[0], Radius=0.9, Where=e))
    want = c.Search(SearchArgs(Vector=q[0], Radius=0.9, Filter=as_filter(e)))
    assert [(r.ID, r.Distance) for r in got.Results] == [(r.ID, r.Distance) for r in want.Results]
    got = c.Search(SearchArgs(Where=e, Limit=7))
    want = c.Search(SearchArgs(Filter=as_filter(e), Limit=7))
    assert [r.ID for r in got.Results] == [r.ID for r in want.Results] and got.PercentSearched == want.PercentSearched


def test_collection_where_equals_filter():
    n = 300
    metas = collection_metadata(n)
    V = orc.synth_vectors(SEED + 5, 0, n + 40, DIM)
    q = orc.synth_vectors(SEED + 6, 0, 3, DIM)
    c = Collection(CollectionOptions(Name="where", DistanceMethod=1, DimensionCount=DIM, Quantization=BITS), devices=[0, 0])
    try:
        c.AddDocuments(range(1000, 1000 + n), V[:n], metas)
        c.IndexField("price", "number")
        c.IndexField("name", "string")
        # the cache: a second call with equal text compiles nothing
        c.Search(SearchArgs(Vector=q[0], K=3, Where=price < 5))
        assert (c.where_compiled, c.where_fallbacks) == (1, 0)
        c.Search(SearchArgs(Vector=q[1], K=3, Where=Field("price") < 5))
        assert (c.where_compiled, c.where_fallbacks) == (1, 0)
        assert_same_answers(c, q, EXPRESSIONS)
        compiled = c.where_compiled   # (the cache keeps 16 entries: the batch may compile some again)
        assert compiled >= len(EXPRESSIONS) and c.where_fallbacks == 0
        # a field that is not indexed, a constant of another type than the index: the Filter path, same answers
        assert_same_answers(c, q, FALLBACKS)
        assert c.where_fallbacks >= len(FALLBACKS) and c.where_compiled == compiled
        with pytest.raises(ValueError):
            c.Search(SearchArgs(Vector=q[0], K=3, Where=price < 5, Filter=lambda i, m: True))
        # a chain of mutations: the columns follow
        c.AddDocument(2000, V[n], b'{"price": 4.5, "name": "ab"}')
        c.AddDocument(2001, V[n + 1], b'not json')
        c.AddDocuments([2002, 2003, 2004], V[n + 2:n + 5], [b'{"name": "zz"}', b'{"price": "5"}', b'[1]'])
        c.AddDocument(1003, V[n + 5], b'{"price": 5, "name": "new"}')   # an existing id: the row is replaced
        c.UpdateDocument(1010, b'{"price": -0.0, "name": "b"}')
        c.UpdateDocument(1011, b'')
        for id_ in (1000, 1064, 1127, 2002):
            c.removeDocument(id_)
        assert_same_answers(c, q, EXPRESSIONS[::3] + FALLBACKS[:1])
        assert c.Compact() == 4
        assert_same_answers(c, q, EXPRESSIONS[1::3])
        c.AddDocument(2005, V[n + 6], b'{"price": 1, "name": "abc"}')
        c.UpdateDocument(2005, b'{"price": 2, "name": "a"}')
        assert_same_answers(c, q, EXPRESSIONS[2::3])
    finally:
        c.Close()
