"""Columns carried across a compaction / reorder on the card (szg_index_reorder_carry / szg_index_compact_carry,
ScanIndex.reorder / compact with ScanColumns in carry=): a carried column reads at new row i exactly what it read at
the old row that became row i -- value bits, present bit, an absent row's stored value or bytes -- and is a live column
afterwards; a text column's heap is repacked, which reclaims dead bytes and dropped rows; refusals leave everything as
it was; the Collection's Compact and re-sort parse no metadata again."""
import numpy as np
import pytest

import oracle as orc
import test_gpu_columns as tgc
import test_gpu_text_columns as tgt
from syzgydb_amd import (Collection, CollectionOptions, Field, ScanIndex, SearchArgs, SzgError, SZG_COSINE, _lib,
                         reorder_plan)

pytestmark = pytest.mark.gpu

SEED, DIM, BITS, SIZES = tgc.SEED, tgc.DIM, tgc.BITS, tgc.SIZES
packed, check_mask, present_variants, loaded_index = tgc.packed, tgc.check_mask, tgc.present_variants, tgc.loaded_index
DROPPED = np.uint64(0xFFFFFFFFFFFFFFFF)
SPECIALS = np.array([0x7FF80000DEADBEEF, 0x8000000000000000, 0, 0x7FF0000000000000, 0xFFF0000000000000,
                     0xFFF8000000000001], dtype=np.uint64).view(np.float64)   # NaN with payload, -0.0, 0.0, inf, -inf, -NaN


def f64_values(n, seed):
    rng = np.random.default_rng(seed)
    v = np.round(rng.normal(0, 10, n), 1)
    where = rng.permutation(n)[:len(SPECIALS)]
    v[where] = SPECIALS[:len(where)]
    return v


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())
    return a.shape == b.shape and bool((a == b).all())


def shard_boundary(n, devices):
    return reorder_plan(n, np.arange(n), len(devices))[0] if devices else None


def three_columns(ix, n, seed):
    """An F64, a U32 and a text column with a non-trivial present pattern each, some rows set absent AFTER creation (so
    they keep a stored value), and what each reads."""
    rng = np.random.default_rng(seed)
    f = ix.column(f64_values(n, seed), present=present_variants(n, seed + 1)[1][1])
    u = ix.column(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), present=rng.random(n) < 0.6)
    t = ix.text_column(tgt.values(n, np.random.default_rng(seed + 2)), present=rng.random(n) < 0.8)
    for col in (f, u, t):
        _, pres = col.read()
        there = np.flatnonzero(pres)
        for row in there[::3][:20]:
            col.set(int(row), None)
    reads = [col.read() for col in (f, u, t)]
    # the absent rows keep what was stored: the test below would not notice a carry that dropped it otherwise
    assert any(len(reads[2][0][i]) for i in range(n) if not reads[2][1][i]) or n < 20
    return [f, u, t], reads


def check_follow(cols, reads, src):
    """Every column reads at new row i what it read at old row src[i]; the text heap holds exactly the carried bytes."""
    src = np.asarray(src, dtype=np.int64)
    for col, (old_v, old_p) in zip(cols, reads):
        new_v, new_p = col.read()
        assert col.rows == len(src)
        assert (new_p == old_p[src]).all()
        if col.kind == _lib.SZG_COL_STR:
            assert new_v == [old_v[s] for s in src]
            info = col.info()
            assert info["heap_used"] == sum(len(v) for v in new_v)
            assert info["kind"] == _lib.SZG_COL_STR and info["rows"] == len(src)
            assert info["heap_capacity"] % 16 == 0 and info["heap_capacity"] >= info["heap_used"] + 16 * bool(len(src))
        else:
            assert bits_equal(new_v, old_v[src])
            assert col.info()["heap_used"] == 0
        if len(src):
            check_mask(col.present(), new_p)   # (the words on the card, and the column is valid)


# ---- 1. reads follow the rows -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("n", SIZES)
def test_reads_follow_the_rows(n, devices):
    rng = np.random.default_rng(n + 31)
    rows = orc.synth_rows(SEED, 0, n, DIM, BITS)
    subset = rng.permutation(n)[:max(1, (2 * n) // 3)]
    dead = set(int(r) for r in np.flatnonzero(rng.random(n) < 0.3)) | {0, n - 1}
    edges = [63, 64]
    b = shard_boundary(n, devices)
    if b is not None:
        edges += [b - 1, b]
    dead |= {r for r in edges if 0 <= r < n}
    for how in ("subset", "reversed", "compact", "empty"):
        with loaded_index(n, devices) as ix:
            cols, reads = three_columns(ix, n, n)
            if how == "subset":
                src = subset
                ix.reorder(src, carry=cols)
            elif how == "reversed":
                src = np.arange(n)[::-1]
                ix.reorder(src, carry=cols)
            elif how == "empty":
                src = np.zeros(0, dtype=np.int64)
                ix.reorder([], carry=cols)
            else:
                for r in sorted(dead):
                    ix.tombstone(r)
                new_of_old = ix.compact(carry=cols)
                src = np.flatnonzero(new_of_old != DROPPED)
                assert sorted(set(range(n)) - dead) == list(src)
            assert ix.rows == len(src)
            assert (ix.read_rows(0, len(src)) == rows[src]).all()
            check_follow(cols, reads, src)
            if len(src) == 0:   # valid columns of 0 rows: they take appended rows like fresh ones
                ix.append(orc.synth_rows(SEED + 1, 0, 3, DIM, BITS))
                cols[0].append([1.0, 2.0, 3.0])
                cols[2].append([b"a", b"", b"xyz"], present=[True, False, True])
                check_mask(cols[0] > 1.5, [False, True, True])
                check_mask(cols[2].contains(b"y"), [False, False, True])


@pytest.mark.parametrize("stage", [592, 1024])
def test_several_windows_per_group(stage):
    """A handle of two shards whose staging window (the handle's test hook carry_stage_bytes) is far smaller than a
    group: values, references and bytes travel in several windows, the last one short.  592 bytes = 37 pieces = 74
    doubles = 148 codes, no multiple of anything else here.  Two destination parts times two source parts make four
    groups, so the largest holds at least a quarter of the rows (and a quarter of the bytes of the 8 windows asserted
    below); in the reversed list every part has ONE group, of all its rows: 388 rows, several windows of codes too."""
    n = 777
    rows = orc.synth_rows(SEED, 0, n, DIM, BITS)
    rng = np.random.default_rng(stage)
    for how in ("subset", "reversed", "compact"):
        with loaded_index(n, [0, 0]) as ix:
            for bad in (24, -16, (64 << 20) + 16):
                with pytest.raises(SzgError):
                    ix.set_option("carry_stage_bytes", bad)
            ix.set_option("carry_stage_bytes", stage)
            cols, reads = three_columns(ix, n, n + 5)
            if how == "subset":
                src = rng.permutation(n)[:600]
                ix.reorder(src, carry=cols)
            elif how == "reversed":   # every row changes its part: each destination part has one group, of all its rows
                src = np.arange(n)[::-1]
                ix.reorder(src, carry=cols)
            else:
                for r in range(0, n, 4):
                    ix.tombstone(r)
                src = np.flatnonzero(ix.compact(carry=cols) != DROPPED)
                assert len(src) == n - (n + 3) // 4
            assert (len(src) + 3) // 4 * 8 > stage and cols[2].info()["heap_used"] > 8 * stage
            assert (ix.read_rows(0, len(src)) == rows[src]).all()
            check_follow(cols, reads, src)


# ---- 2. a carried column is a live column -------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_carried_column_is_live(devices):
    n, m, extra = 2200, 2040, 70   # m rows are kept: 70 more cross the capacity step of the (last) part, 2048 / 1024 rows
    rng = np.random.default_rng(77)
    all_rows = orc.synth_rows(SEED, 0, n + extra, DIM, BITS)
    v = f64_values(n + extra, 78)
    codes = rng.integers(0, 50, n + extra).astype(np.uint32)
    text = tgt.values(n + extra, np.random.default_rng(79))
    pres = rng.random(n + extra) < 0.7
    base_bool = rng.random(n) < 0.6
    src = rng.permutation(n)[:m]
    with ScanIndex(DIM, BITS, SZG_COSINE, devices=devices) as ix, np.errstate(invalid="ignore"):
        ix.load(all_rows[:n])
        f = ix.column(v[:n], present=pres[:n])
        u = ix.column(codes[:n], present=pres[:n])
        t = ix.text_column(text[:n], present=pres[:n])
        base = ix.mask(base_bool)
        ix.reorder(src, carry=[f, base, u, t])   # masks and columns in one list
        order = np.concatenate([src, np.arange(n, n + extra)])
        v, codes, pres = v[order], codes[order], pres[order]
        text = [text[i] for i in order]
        bb = base_bool[src]
        assert (base.read() == packed(bb)).all() and base.count == int(bb.sum())
        allowed = np.arange(50) % 3 == 0
        constants = tgt.constants_for(text[:m])[:8] + [tgt.NEEDLE]

        def verify(rows, bm, bbool):
            for op, fn in tgc.OPS.items():
                for c in (0.0, 2.5):
                    check_mask(f.where(op, c, base=bm), fn(v[:rows], c) & pres[:rows] & bbool, (op, c))
            check_mask(f.isin([0.0, 2.5, np.nan], base=bm), np.isin(v[:rows], [0.0, 2.5]) & pres[:rows] & bbool)
            check_mask(u.codes(allowed, base=bm), allowed[codes[:rows]] & pres[:rows] & bbool)
            for col in (f, u, t):
                check_mask(col.present(base=bm), pres[:rows] & bbool)
            for op, fn in tgt.OPS.items():
                for c in constants:
                    want = np.array([fn(x, c) for x in text[:rows]]) & pres[:rows] & bbool
                    check_mask(tgt.where(t, op, c, base=bm), want, (op, c))

        verify(m, base, bb)
        # rows behind the carried ones: the index first, then every column -- the part grows past its capacity
        ix.append(all_rows[n:])
        for col, vals in ((f, v[m:]), (u, codes[m:]), (t, text[m:])):
            with pytest.raises(SzgError) as e:
                col.present()
            assert "short column" in str(e.value)
            col.append(vals, present=pres[m:])
        total = m + extra
        everything = np.ones(total, bool)
        verify(total, None, everything)
        # single rows, the same ones in every column: a shorter text in place, a longer one to the heap's end, a row
        # at a word boundary, and one marked absent
        def set_all(r, number, code, string):
            f.set(r, number), u.set(r, code), t.set(r, string)
            if string is None:
                pres[r] = False
            else:
                v[r], codes[r], text[r], pres[r] = number, code, string, True

        used = t.info()["heap_used"]
        shrunk = next(i for i in range(m) if len(text[i]) >= 8 and pres[i])
        set_all(shrunk, 2.5, 3, b"xy")
        assert t.info()["heap_used"] == used
        longer = next(i for i in range(m) if len(text[i]) < 100 and i != shrunk)
        set_all(longer, -0.0, 49, b"L" * 400 + tgt.NEEDLE)
        assert t.info()["heap_used"] == used + 400 + len(tgt.NEEDLE)
        set_all(64, np.nan, 0, b"")
        set_all(total - 1, None, None, None)
        verify(total, None, everything)
        got_v, got_p = t.read()
        assert (got_p == pres).all() and all(got_v[i] == text[i] for i in range(total) if pres[i])


# ---- 3. reclaim -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_compaction_reclaims_the_text_heap(devices):
    n = 400
    rng = np.random.default_rng(5)
    text = tgt.values(n, np.random.default_rng(6))
    with loaded_index(n, devices) as ix:
        col = ix.text_column(text)
        fresh = col.info()
        assert fresh["heap_used"] == sum(len(x) for x in text)
        grown = rng.permutation(n)[:50]
        dead_bytes = 0
        for row in grown:   # each goes to the heap's end: the old bytes are dead
            dead_bytes += len(text[row])
            text[row] = text[row] + b"-grown-%d" % int(row)
            col.set(int(row), text[row])
        before = col.info()
        assert before["heap_used"] == sum(len(x) for x in text) + dead_bytes and dead_bytes > 0
        dead = rng.permutation(n)[:n // 4]
        for row in dead:
            ix.tombstone(int(row))
        new_of_old = ix.compact(carry=[col])
        keep = np.flatnonzero(new_of_old != DROPPED)
        after = col.info()
        assert after["rows"] == n - len(dead) == col.rows
        assert after["heap_used"] == sum(len(text[r]) for r in keep) < before["heap_used"] - dead_bytes
        assert after["device_bytes"] <= before["device_bytes"] and after["heap_capacity"] <= before["heap_capacity"]
        got_v, got_p = col.read()
        assert got_v == [text[r] for r in keep] and got_p.all()
        check_mask(col.contains(b"-grown-"), np.array([b"-grown-" in text[r] for r in keep]))


# ---- 4. the scan of the lengths across blocks -------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_scan_across_blocks(devices):
    """70 000 short strings: the compacted rows span more blocks of the lengths' scan than its second level takes in
    one step, in a handle of one shard and in each group of a handle of two."""
    n = 70000
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 9, n)
    letters = rng.integers(97, 123, int(lens.sum()), dtype=np.uint8).tobytes()
    ends = np.cumsum(lens)
    text = [letters[int(e - l):int(e)] for e, l in zip(ends, lens)]
    text[40001] = b"q" * 4990 + tgt.NEEDLE
    with loaded_index(n, devices) as ix:
        col = ix.text_column(text)
        keep = np.flatnonzero(np.arange(n) % 3 != 0)
        for row in range(0, n, 3):
            ix.tombstone(row)
        new_of_old = ix.compact(carry=[col])
        assert (np.flatnonzero(new_of_old != DROPPED) == keep).all()
        got_v, got_p = col.read()
        assert col.rows == len(keep) and got_p.all()
        assert got_v == [text[r] for r in keep]
        assert col.info()["heap_used"] == sum(len(text[r]) for r in keep)
        m = col.contains(tgt.NEEDLE)
        assert m.count == 1 and list(np.flatnonzero(np.unpackbits(m.read().view(np.uint8), bitorder="little"))) == \
            [int(np.searchsorted(keep, 40001))]
        m.close()


def watch_index(index, dead_row, n, text, keep_bool):
    """A valid text column and a valid mask of `index`, one row tombstoned, and a check that the rows, the
    live bits, the column and the mask are what they are now, and still valid."""
    good = index.text_column(text, present=np.arange(n) % 2 == 0)
    mask = index.mask(keep_bool)
    index.tombstone(dead_row)
    state = (good.read(), good.info(), mask.read().copy(), index.read_rows(0, n).copy())

    def unchanged():
        assert index.rows == n and index.live_rows == n - 1
        assert (index.read_rows(0, n) == state[3]).all()
        got = good.read()
        assert got[0] == state[0][0] and (got[1] == state[0][1]).all() and good.info() == state[1]
        check_mask(good.present(), state[0][1])   # still valid
        assert (mask.read() == state[2]).all()
        check_mask(good.present(base=mask), state[0][1] & keep_bool)   # the mask as well

    return good, mask, unchanged


# ---- 5. refusals and atomicity ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_refusals_leave_everything_as_it_was(devices):
    n = 300
    rows = orc.synth_rows(SEED, 0, n + 1, DIM, BITS)
    text = tgt.values(n, np.random.default_rng(3))
    v = f64_values(n, 4)
    keep_bool = np.arange(n) % 5 != 0
    with loaded_index(n, devices) as ix, loaded_index(n, devices) as other, loaded_index(n, devices) as moved:
        # a stale column of its index: made before a reorder that did not carry it
        stale = moved.column(v)
        moved.reorder(np.arange(n)[::-1])
        assert stale.info()["rows"] == n and stale.info()["kind"] == _lib.SZG_COL_F64   # info works on a stale column
        foreign = other.column(v)
        short = ix.column(v[:n - 10])

        def watch(index, dead_row):
            return watch_index(index, dead_row, n, text, keep_bool)

        good, mask, unchanged = watch(ix, 7)
        moved_good, moved_mask, moved_unchanged = watch(moved, 9)   # (made after the reorder: valid beside the stale one)
        for bad, word, owner, ok, msk, same in ((short, "short column", ix, good, mask, unchanged),
                                                (foreign, "another handle", ix, good, mask, unchanged),
                                                (stale, "stale column", moved, moved_good, moved_mask, moved_unchanged)):
            for call in (lambda: owner.compact(carry=[msk, ok, bad]), lambda: owner.reorder([3, 2, 1], carry=[msk, ok, bad])):
                with pytest.raises(SzgError) as e:
                    call()
                assert e.value.code == _lib.SZG_E_INVALID and word in str(e.value)
                same()
        assert stale.info()["rows"] == n
        # a bad row in the list, with good columns in carry: nothing moves either
        with pytest.raises(SzgError):
            ix.reorder([1, 1], carry=[good])
        with pytest.raises(SzgError):
            ix.reorder([7], carry=[good])   # a tombstoned row
        unchanged()
        short.close()
        # a duplicate is taken once; the old call still makes a column stale; without tombstones nothing moves
        with loaded_index(n, devices) as ix2:
            a, b = ix2.text_column(text), ix2.column(v)
            info = a.info()
            ix2.compact(carry=[a, a])
            assert a.info() == info and a.rows == n
            check_mask(a.present(), np.ones(n, bool))
            check_mask(b.present(), np.ones(n, bool))   # no tombstones: not carried, and still valid
            ix2.tombstone(0)
            ix2.compact(carry=[a, a])
            assert a.rows == n - 1 and a.read()[0] == text[1:]
            carried = a.info()
            assert carried["rows"] == n - 1 and carried["heap_used"] == sum(len(x) for x in text[1:])
            with pytest.raises(SzgError) as e:   # b was not in the list
                b.present()
            assert "stale column" in str(e.value)
            ix2.tombstone(0)
            ix2.compact()
            with pytest.raises(SzgError) as e:
                a.present()
            assert e.value.code == _lib.SZG_E_INVALID and "stale column" in str(e.value)
            assert a.rows == n - 1 and a.info() == carried   # a stale column keeps what it had, and info() reports it


# ---- 6. the Collection -------------------------------------------------------------------------------------------------

price, brand, email = Field("price"), Field("brand"), Field("email")
EXPRESSIONS = [price < 5, price != 2.5, brand == "b", brand.isin(["a", "zz"]), email.startswith("user1"),
               email.contains("7@"), email.endswith("3@example.org"), (price < 3) & (brand != "a"),
               email.contains("er2") | (price >= 5), ~(email < "user5"), email == "user42@example.org"]


def metadata(i):
    if i % 17 == 0:
        return b"not json"
    if i % 13 == 0:
        return b'{"price": "n/a", "brand": 7}'
    return ('{"price": %s, "brand": "%s", "email": "user%d@example.org"}'
            % ((i % 12) * 0.5, ["a", "ab", "b", "zz", ""][i % 5], i)).encode()


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_collection_carries_its_columns(devices):
    n = 200
    V = orc.synth_vectors(SEED + 5, 0, n + 2, DIM)
    q = orc.synth_vectors(SEED + 6, 0, 3, DIM)
    same = tgc.assert_same_answers
    c = Collection(CollectionOptions(Name="carry", DistanceMethod=1, DimensionCount=DIM, Quantization=BITS), devices=devices,
                   auto_compact=0.25)
    try:
        c.AddDocuments(range(1000, 1000 + n), V[:n], [metadata(i) for i in range(n)])
        c.IndexField("price", "number")
        c.IndexField("brand", "string")
        c.IndexField("email", "text")
        c.UpdateDocument(1003, b'{"price": 1, "brand": "ab", "email": "a much longer address than before <user3@example.org>"}')
        same(c, q, EXPRESSIONS)
        assert c.where_fallbacks == 0
        used = c._fields["email"].column.info()["heap_used"]
        rng = np.random.default_rng(8)
        victims = [int(i) for i in 1000 + rng.permutation(n)]
        removed = 0
        while c.compactions < 2:
            c.removeDocument(victims[removed])
            removed += 1
            if removed in (20, 60):
                same(c, q, EXPRESSIONS[::2])
        assert removed == 51 + 38 and c.compactions == 2 and c.column_rebuilds == 0
        assert c._index.rows == n - removed == c._fields["email"].column.rows
        assert c._fields["email"].column.info()["heap_used"] < used
        same(c, q, EXPRESSIONS)
        assert c.where_fallbacks == 0
        # the columns go on following the collection
        c.AddDocument(3000, V[n], b'{"price": 0.5, "brand": "zz", "email": "user7@late.example.org"}')
        c.UpdateDocument(3000, b'{"price": 4, "brand": "new brand", "email": "x"}')
        same(c, q, EXPRESSIONS[1::2] + [brand == "new brand"])
        # the lazy re-sort: an id that sorts before the last one, then a batch
        c.AddDocument(100, V[n + 1], b'{"price": 2.5, "brand": "b", "email": "user100@example.org"}')
        assert c._order_stale and c.resorts == 0
        same(c, q, EXPRESSIONS)
        assert c.resorts == 1 and not c._order_stale
        assert c.column_rebuilds == 0 and c.compactions == 2 and c.where_fallbacks == 0
        assert c._id_of[0] == 100 and c._fields["email"].column.read()[0][0] == b"user100@example.org"
    finally:
        c.Close()
