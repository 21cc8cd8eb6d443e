"""Text columns (SZG_COL_STR / ScanIndex.text_column): the strings' bytes live on the card beside the rows and
szg_mask_where_str compares them against a constant in one kernel per shard.  The words and counts are checked against
Python's own bytes operations at the sizes of test_gpu_columns.py, with values of every length class the predicate
treats differently (empty, below a dword, across dwords, 300 and 4998 bytes) over an alphabet with NUL, 0xff and a
two-byte UTF-8 letter; then append and set, staleness and kinds, the mask as an ordinary mask, and a Collection whose
`name` field is indexed as "text" against the Filter path."""
import ctypes

import numpy as np
import pytest

import oracle as orc
import test_gpu_columns as tgc
from syzgydb_amd import Collection, CollectionOptions, Field, ScanIndex, SearchArgs, SzgError, SZG_COSINE, _lib

pytestmark = pytest.mark.gpu

SEED, DIM, BITS, SIZES = tgc.SEED, tgc.DIM, tgc.BITS, tgc.SIZES
packed, check_mask, present_variants, loaded_index = tgc.packed, tgc.check_mask, tgc.present_variants, tgc.loaded_index

ALPHA = [b"a", b"b", b"\x00", b"\xc3\xa9", b"\xff"]
LENS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 64, 300]
NEEDLE = b"needle\xffz"


def values(n, rng):
    out = []
    for i in range(n):
        L = LENS[rng.integers(len(LENS))]
        out.append(b"".join(ALPHA[j] for j in rng.integers(0, len(ALPHA), L))[:L])
    if n >= 65:
        out[1], out[2] = b"ab", b"cd"
    if n >= 129:
        out[100] = b"a" * 4990 + NEEDLE
    return out


OPS = {
    "==": lambda v, c: v == c, "!=": lambda v, c: v != c, "<": lambda v, c: v < c, "<=": lambda v, c: v <= c,
    ">": lambda v, c: v > c, ">=": lambda v, c: v >= c,
    "startswith": lambda v, c: v.startswith(c), "endswith": lambda v, c: v.endswith(c), "contains": lambda v, c: c in v,
}


def where(col, op, constant, base=None):
    if op in ("startswith", "endswith", "contains"):
        return getattr(col, op)(constant, base=base)
    return col.where(op, constant, base=base)


def constants_for(vals):
    out = [b"", b"a", b"ab", b"\x00", b"\xc3\xa9", b"\xff"]
    middle = sorted(v for v in vals if 4 <= len(v) <= 64)
    if middle:
        stored = middle[len(middle) // 2]
        out += [stored, stored[:-1], stored + b"a", stored[1:]]
    out += [b"bc", NEEDLE]
    long_ones = [v for v in vals if len(v) == 300]
    if long_ones:
        head = long_ones[0][:256]
        out += [head, head[:-1] + (b"b" if head[-1:] != b"b" else b"a")]
    return out


_CASES = {}


def case(n):
    """(values, constants, Python's verdicts per (op, constant)) for one size: computed once, shared, never changed."""
    if n not in _CASES:
        vals = values(n, np.random.default_rng(n))
        consts = constants_for(vals)
        truth = {(op, i): np.array([fn(v, c) for v in vals], dtype=bool)
                 for op, fn in OPS.items() for i, c in enumerate(consts)}
        for t in truth.values():
            t.setflags(write=False)
        _CASES[n] = (vals, consts, truth)
    return _CASES[n]


# ---- 1. words and counts against Python -----------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("n", SIZES)
def test_str_words_and_counts(n, devices):
    vals, consts, truth = case(n)
    with loaded_index(n, devices) as ix:
        base_bool = np.random.default_rng(n + 7).random(n) < 0.6
        if n >= 129:
            base_bool[100] = True
        base = ix.mask(base_bool)
        for pname, parg, pres in present_variants(n, n + 1):
            with ix.text_column(vals, present=parg) as col:
                assert col.rows == n and col.kind == _lib.SZG_COL_STR
                got_v, got_p = col.read()
                assert (got_p == pres).all()
                assert all(got_v[i] == vals[i] for i in range(n) if pres[i]), pname
                for bm, bb in ((None, np.ones(n, bool)), (base, base_bool)):
                    for op in OPS:
                        inside = 0
                        for i, c in enumerate(consts):
                            want = truth[(op, i)] & pres & bb
                            inside += 0 < int(want.sum()) < n
                            check_mask(where(col, op, c, base=bm), want, (pname, op, c, bm is not None))
                        if n >= 63 and pname == "none" and bm is None:
                            # (so the test cannot pass on empty or full masks alone)
                            assert inside >= 3, (op, inside)
                    check_mask(col.present(base=bm), pres & bb, pname)
                    # rows 1 and 2 are b"ab" and b"cd", adjacent in the heap: no row contains b"bc"
                    m = col.contains(b"bc", base=bm)
                    assert m.count == 0
                    m.close()
                    if n >= 129:
                        m = col.contains(NEEDLE, base=bm)
                        assert m.count == int(pres[100])   # (row 100 is in the base)
                        m.close()
                check_mask(col < b"b", np.array([v < b"b" for v in vals]) & pres)
                check_mask(col.eq("é"), np.array([v == b"\xc3\xa9" for v in vals]) & pres)   # (a str: its UTF-8 bytes)


# ---- 2. append and set ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_append_and_set(devices):
    rng = np.random.default_rng(11)
    blocks = [100, 37, 129, 71]
    total = sum(blocks)
    all_rows = orc.synth_rows(SEED, 0, total, DIM, BITS)
    vals = values(total, np.random.default_rng(12))
    vals[64] = b"xy"
    pres = rng.random(total) < 0.7
    pres[[5, 64, total - 1]] = True
    pres[[6, 63]] = False

    def verify(col, n, eq_constant, contains_constant):
        got_v, got_p = col.read()
        assert col.rows == n and len(got_v) == n and (got_p == pres[:n]).all()
        assert all(got_v[i] == vals[i] for i in range(n) if pres[i])   # (an absent row's stored value is not defined)
        check_mask(col.where("==", eq_constant), np.array([v == eq_constant for v in vals[:n]]) & pres[:n])
        check_mask(col.contains(contains_constant), np.array([contains_constant in v for v in vals[:n]]) & pres[:n])

    with ScanIndex(DIM, BITS, SZG_COSINE, devices=devices) as ix:
        ix.load(all_rows[:100])
        col = ix.text_column(vals[:100], present=pres[:100])
        verify(col, 100, vals[5], b"ab")
        at = 100
        for step, count in enumerate(blocks[1:]):
            ix.append(all_rows[at:at + count])
            with pytest.raises(SzgError) as e:   # shorter than the index until appended
                col.contains(b"a")
            assert e.value.code == _lib.SZG_E_INVALID and "short column" in str(e.value)
            if step == 0:     # present bits relative to the block: an unaligned shift
                col.append(vals[at:at + count], present=pres[at:at + count])
            elif step == 1:   # as words; across pairs, and a shard's growth
                col.append(vals[at:at + count], present=packed(pres[at:at + count]))
            else:             # None marks the absent rows
                col.append([v if p else None for v, p in zip(vals[at:at + count], pres[at:at + count])])
            at += count
            verify(col, at, vals[at - 1][:256], NEEDLE)
        with pytest.raises(SzgError) as e:
            col.append([b"x"])
        assert e.value.code == _lib.SZG_E_RANGE
        verify(col, total, vals[1], b"\xff\x00")   # an error leaves the column as it was
        # one row through every case of set; the dead bytes behind a shortened value must not be found
        row = 64
        for value, gone in ((b"0123456789ABCDEFGHIJ", None),        # longer than what was there: out of line
                            (b"01234", b"56789"),                   # shorter: in place
                            (b"abcde", b"01234"),                   # equal length: in place
                            (b"abcde" * 40 + b"\x00\xff", None),    # longer again
                            (b"", b"abcde")):                       # empty
            col.set(row, value)
            vals[row] = value
            verify(col, total, value, value[2:7])
            if gone is not None:
                m = col.contains(gone)
                assert m.count == sum(gone in v for v, p in zip(vals, pres) if p)
                assert not (int(m.read()[row // 64]) >> (row % 64)) & 1
                m.close()
        col.set(row, None)
        pres[row] = False
        verify(col, total, b"", b"a")
        for absent_row, value in ((63, b"was absent"), (6, b"")):   # formerly absent rows (length 0 at creation)
            col.set(absent_row, value)
            vals[absent_row], pres[absent_row] = value, True
            verify(col, total, value, b"absent")
        for last in (0, total - 1):
            col.set(last, "été")   # a str: its UTF-8 bytes
            vals[last] = "été".encode()
            verify(col, total, vals[last], b"\xa9t")
        with pytest.raises(SzgError) as e:
            col.set(total, b"x")
        assert e.value.code == _lib.SZG_E_RANGE


# ---- 3. staleness and kinds -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["load", "synth", "reorder", "compact"])
def test_stale_text_column(how):
    n = 200
    vals = values(n, np.random.default_rng(14))
    present = np.arange(n) % 2 == 0
    with loaded_index(n, [0, 0]) as ix:
        col = ix.text_column(vals, present=present)
        if how == "load":
            ix.load(orc.synth_rows(SEED + 1, 0, n, DIM, BITS))
        elif how == "synth":
            ix.synth(n, 5)
        elif how == "reorder":
            ix.reorder(np.arange(n)[::-1])
        else:
            ix.tombstone(7)
            ix.compact()
        for call in (lambda: col.where("==", b"a"), lambda: col.contains(b"a"), lambda: col.present(),
                     lambda: col.append([b"a"]), lambda: col.set(0, b"a"), lambda: col.set(0, None)):
            with pytest.raises(SzgError) as e:
                call()
            assert e.value.code == _lib.SZG_E_INVALID and "stale column" in str(e.value)
        assert col.rows == n
        got_v, got_p = col.read()
        assert (got_p == present).all() and all(got_v[i] == vals[i] for i in range(n) if present[i])
        col.close()


def test_kinds_do_not_mix_and_limits():
    n = 130
    vals = values(n, np.random.default_rng(15))
    ix = loaded_index(n, None)
    other = loaded_index(n, None)
    try:
        L = ix._L
        text = ix.text_column(vals)
        numbers = ix.column(np.arange(n, dtype=np.float64))
        codes = ix.column(np.arange(n, dtype=np.uint32))
        one = (ctypes.c_double * 1)(1.0)
        bits = (ctypes.c_uint64 * 1)(1)
        out = ctypes.c_void_p(0x1234)
        buf = (ctypes.c_double * n)()
        # the calls of the other kinds on a text column
        for rc in (L.szg_column_append(text._h, one, None, 0), L.szg_column_set(text._h, 0, one),
                   L.szg_column_read(text._h, 0, n, buf, None),
                   L.szg_mask_where_f64(text._h, _lib.SZG_CMP_LT, 1.0, None, ctypes.byref(out)),
                   L.szg_mask_where_in_f64(text._h, one, 1, None, ctypes.byref(out)),
                   L.szg_mask_where_u32(text._h, bits, 1, None, ctypes.byref(out))):
            assert rc == _lib.SZG_E_INVALID and b"kind does not match" in L.szg_last_error()
        for call in (lambda: text.where("<", 1.0), lambda: text.isin([1.0]), lambda: text.codes([True])):
            with pytest.raises(SzgError) as e:
                call()
            assert e.value.code == _lib.SZG_E_INVALID
        # ... and the text calls on the other kinds
        chars = (ctypes.c_uint8 * 1)(97)
        offsets = (ctypes.c_uint64 * 2)(0, 1)
        for c in (numbers, codes):
            for rc in (L.szg_column_append_str(c._h, chars, offsets, None, 0), L.szg_column_set_str(c._h, 0, chars, 1),
                       L.szg_column_read_str(c._h, 0, n, None, None, 0, None),
                       L.szg_mask_where_str(c._h, _lib.SZG_STR_CONTAINS, chars, 1, None, ctypes.byref(out))):
                assert rc == _lib.SZG_E_INVALID and b"kind does not match" in L.szg_last_error()
            for call in (lambda: c.where("==", b"a"), lambda: c.contains("a"), lambda: c.startswith(b"a")):
                with pytest.raises(SzgError) as e:
                    call()
                assert e.value.code == _lib.SZG_E_INVALID
        assert out.value == 0x1234
        # what works on every kind
        words = (ctypes.c_uint64 * ((n + 63) // 64))()
        assert L.szg_column_read(text._h, 0, n, None, words) == _lib.SZG_OK and text.rows == n
        check_mask(text.present(), np.ones(n, bool))
        # szg_column_read_str: the offsets alone, then a buffer that is too small
        offs = (ctypes.c_uint64 * (n + 1))()
        assert L.szg_column_read_str(text._h, 0, n, offs, None, 0, None) == _lib.SZG_OK
        assert list(offs) == list(np.concatenate([[0], np.cumsum([len(v) for v in vals])]))
        small = (ctypes.c_uint8 * 8)()
        offs2 = (ctypes.c_uint64 * (n + 1))()
        assert L.szg_column_read_str(text._h, 0, n, offs2, small, 8, None) == _lib.SZG_E_TRUNCATED
        assert list(offs2) == list(offs)
        # the constant's limit, the operators
        check_mask(text.contains(b"a" * 256), np.array([b"a" * 256 in v for v in vals]))
        with pytest.raises(SzgError) as e:
            text.contains(b"a" * 257)
        assert e.value.code == _lib.SZG_E_UNSUPPORTED
        with pytest.raises(SzgError) as e:
            text.where(9, b"a")
        assert e.value.code == _lib.SZG_E_INVALID and "operator" in str(e.value)
        with pytest.raises(SzgError) as e:
            ix.column(np.zeros(n), kind=_lib.SZG_COL_F64).where(_lib.SZG_STR_CONTAINS, 1.0)   # not an f64 operator
        assert e.value.code == _lib.SZG_E_INVALID
        # base masks: closed, of another handle, stale
        closed = ix.mask(np.ones(n, bool))
        closed.close()
        with pytest.raises(ValueError):
            text.contains(b"a", base=closed)
        foreign = other.mask(np.ones(n, bool))
        with pytest.raises(SzgError) as e:
            text.contains(b"a", base=foreign)
        assert e.value.code == _lib.SZG_E_INVALID
        old = ix.mask(np.ones(n, bool))
        ix.append(orc.synth_rows(SEED + 2, 0, 1, DIM, BITS))   # `old` is stale now, the column short
        text.append([b"late"])
        with pytest.raises(SzgError) as e:
            text.contains(b"a", base=old)
        assert e.value.code == _lib.SZG_E_INVALID and "stale mask" in str(e.value)
        check_mask(text.endswith(b"ate"), np.array([v.endswith(b"ate") for v in vals + [b"late"]]))
    finally:
        other.close()
        ix.close()   # with live columns and masks: they are closed first
    assert not text._h and not numbers._h


# ---- 4. the mask is an ordinary mask ----------------------------------------------------------------------------------

def test_text_mask_algebra_compaction_and_search():
    n, k = 2048, 10
    rows = orc.synth_rows(SEED, 0, n, DIM, BITS)
    vals = values(n, np.random.default_rng(4))
    has = np.array([b"ab" in v for v in vals])
    assert 0 < has.sum() < n
    other_bool = np.random.default_rng(5).random(n) < 0.5
    with loaded_index(n, [0, 0]) as ix:
        col = ix.text_column(vals)
        other = ix.mask(other_bool)
        m = col.contains(b"ab")
        check_mask(m & other, has & other_bool)
        check_mask(~m, ~has)
        check_mask(col.startswith(b"a") | other, np.array([v.startswith(b"a") for v in vals]) | other_bool)
        live0 = ix.mask_stats()["live_masks"]
        extra = col.where(">=", b"b")
        assert ix.mask_stats()["live_masks"] == live0 + 1   # accounted like every mask
        extra.close()
        # a top-k search with it: the same ids and float64 distances as with a mask made from the same bits
        same = ix.mask(has)
        Q = orc.synth_vectors(SEED + 1, 0, 3, DIM)
        r, d, c = ix.search_topk(Q, k, masks=m)
        r2, d2, c2 = ix.search_topk(Q, k, masks=same)
        assert (c == c2).all() and (r == r2).all() and (d.view(np.uint64) == d2.view(np.uint64)).all()
        o_rows, o_dist, _ = orc.search_exact(rows, DIM, BITS, SZG_COSINE, Q[0], k=k, allow=has.astype(np.uint8))
        assert list(map(int, r[0, : c[0]])) == list(map(int, o_rows))
        assert (d[0, : c[0]].view(np.uint64) == np.asarray(o_dist, dtype=np.float64).view(np.uint64)).all()
        # carried across a compaction that moves rows
        dead = [0, 63, 64, 1000, n - 1]
        for row in dead:
            ix.tombstone(row)
        new_of_old = ix.compact(carry=[m])
        keep = np.flatnonzero(new_of_old != np.uint64(0xFFFFFFFFFFFFFFFF))
        assert ix.rows == n - len(dead)
        assert (m.read() == packed(has[keep])).all() and m.count == int(has[keep].sum())


# ---- 5. the Collection ------------------------------------------------------------------------------------------------

price, name = Field("price"), Field("name")


def test_collection_text_field_equals_filter():
    n = 300
    metas = tgc.collection_metadata(n)
    V = orc.synth_vectors(SEED + 5, 0, n + 40, DIM)
    q = orc.synth_vectors(SEED + 6, 0, 3, DIM)
    same = tgc.assert_same_answers
    c = Collection(CollectionOptions(Name="text", DistanceMethod=1, DimensionCount=DIM, Quantization=BITS), devices=[0, 0])
    try:
        c.AddDocuments(range(1000, 1000 + n), V[:n], metas)
        c.IndexField("price", "number")
        c.IndexField("name", "text")
        assert c._fields["name"].column.kind == _lib.SZG_COL_STR and not c._fields["name"].codes
        same(c, q, tgc.EXPRESSIONS)
        compiled = c.where_compiled   # (the cache keeps 16 entries: the batch may compile some again)
        assert compiled >= len(tgc.EXPRESSIONS) and c.where_fallbacks == 0
        same(c, q, [name.isin(["a", "zz", "a", "b"]), name.notin(["a", "ab"]), name.isin([]), name.contains(""),
                    name == "", name >= ""])
        assert c.where_fallbacks == 0
        compiled = c.where_compiled
        # a field that is not indexed, a constant of another type than the index: the Filter path, same answers
        same(c, q, tgc.FALLBACKS)
        fallbacks = c.where_fallbacks
        assert fallbacks >= len(tgc.FALLBACKS) and c.where_compiled == compiled
        # beyond the kernel's limits: an IN-list of 17 strings, a 257-byte constant
        beyond = [name.isin(["abc"] + ["n%d" % i for i in range(16)]), name.contains("a" * 257), name != "b" * 257]
        same(c, q, beyond)
        assert c.where_fallbacks >= fallbacks + len(beyond) and c.where_compiled == compiled
        # a chain of mutations: the columns follow
        c.AddDocument(2000, V[n], b'{"price": 4.5, "name": "ab"}')
        c.AddDocument(2001, V[n + 1], b'not json')
        c.AddDocuments([2002, 2003, 2004], V[n + 2:n + 5], [b'{"name": "zz"}', b'{"price": "5"}', b'[1]'])
        c.AddDocument(1003, V[n + 5], b'{"price": 5, "name": "new"}')   # an existing id: the row is replaced
        c.UpdateDocument(1010, b'{"price": -0.0, "name": "b"}')
        c.UpdateDocument(1011, b'')
        c.UpdateDocument(1012, b'{"price": 1, "name": "abc, but a much longer name than the row held before"}')
        c.UpdateDocument(1013, b'{"price": 1, "name": "a"}')
        c.UpdateDocument(1012, b'{"price": 1, "name": "ab"}')   # shorter again: in place
        for id_ in (1000, 1064, 1127, 2002):
            c.removeDocument(id_)
        same(c, q, tgc.EXPRESSIONS[::3] + tgc.FALLBACKS[:1] + [name.contains("longer"), name.endswith("before")])
        assert c.Compact() == 4
        same(c, q, tgc.EXPRESSIONS[1::3])
        c.AddDocument(2005, V[n + 6], b'{"price": 1, "name": "abc"}')
        c.UpdateDocument(2005, b'{"price": 2, "name": "a"}')
        same(c, q, tgc.EXPRESSIONS[2::3])
    finally:
        c.Close()
