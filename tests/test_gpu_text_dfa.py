"""szg_mask_where_dfa / ScanColumn.dfa / ScanColumn.matches / Field.matches on the card: a byte automaton walked over
each row of a text column by one kernel per shard.  Hand-built automata test the kernel apart from the pattern compiler
(verdicts from a bytewise walker in Python); compiled patterns are checked against Python's `re`; a trie of 300 strings
runs through the global-memory tier and a smaller one through the LDS tier; then the refusals on a live column, and a
Collection whose `email` field is indexed as "text" (and `name` as "string") against the Filter path.  Sizes, present
variants and the mask check are test_gpu_columns.py's, the values test_gpu_text_columns.py's: lengths 0 to 300 over an
alphabet with NUL, 0xff and a two-byte UTF-8 letter, and a 5 KB row."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle as orc
import test_gpu_columns as tgc
import test_gpu_text_columns as tgt
from test_regex_dfa_cpu import DOTTED_QUAD, EMAIL, to_python
from syzgydb_amd import Collection, CollectionOptions, Field, SearchArgs, SzgError, _lib, regex_dfa

pytestmark = pytest.mark.gpu

SEED, DIM, BITS, SIZES = tgc.SEED, tgc.DIM, tgc.BITS, tgc.SIZES
check_mask, present_variants, loaded_index = tgc.check_mask, tgc.present_variants, tgc.loaded_index
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the planted rows hold: each compiled pattern matches some of them
PLANTED = [b"someone@example.org", b"a@d.cd", b"\xc3\xa9@\xe2\x82\xac.info", b"x.y@z.museum", b"q@q.qq",
           b"1.2.3.4", b"192.168.1.255", b"0.0.0.0", b"10.20.30.40", b"999.9.99.0",
           b"xx needle", b"needle", b"the needle in it", b"a" * 290 + b"needle", b"needlework\n",
           b"abab", b"ababab", b"xabab", b"abababab", b"(abab)",
           b"tab\there", b"line\nbreak", b"two  spaces", b" ", b"\r\n"]


def values(n):
    """test_gpu_text_columns.values -- rows 1 and 2 are b"ab" and b"cd", row 100 is 5 KB -- with the planted rows laid
    over it from row 130 on, 7 apart."""
    out = tgt.values(n, np.random.default_rng(n))
    for i, v in enumerate(PLANTED):
        if 130 + 7 * i < n:
            out[130 + 7 * i] = v
    return out


def walk(d, v):
    """The bytewise walker: every byte, one transition."""
    s = d.start
    for b in v:
        s = int(d.next[s, d.class_of[b]])
    return bool(d.accept[s])


def automaton(n_states, classes, table, accept, start=0):
    """classes: {byte: class}, every other byte is class 0"""
    class_of = np.zeros(256, dtype=np.uint8)
    for b, c in classes.items():
        class_of[b] = c
    return regex_dfa.Dfa(class_of, np.array(table, dtype=np.uint16).reshape(n_states, -1), np.array(accept, dtype=bool), start)


HAND_BUILT = [
    # no absorbing state: every byte of every row is read
    ("length = 0 mod 3", automaton(3, {}, [1, 2, 0], [True, False, False]), lambda v: len(v) % 3 == 0),
    ("odd number of 0xff", automaton(2, {0xff: 1}, [0, 1, 1, 0], [False, True]), lambda v: v.count(b"\xff") % 2 == 1),
    # an absorbing accept
    ("contains NUL", automaton(2, {0: 1}, [0, 1, 1, 1], [False, True]), lambda v: b"\x00" in v),
    # absorbing from byte 1 either way, on the 5 KB row as well; started elsewhere than in state 0
    ("first byte is a", automaton(3, {0x61: 1}, [0, 0, 1, 1, 0, 1], [False, True, False], start=2), lambda v: v[:1] == b"a"),
    ("rejects all", automaton(1, {}, [0], [False]), lambda v: False),
    ("accepts all", automaton(1, {}, [0], [True]), lambda v: True),
]

_CASES = {}


def case(n):
    """(values, the walker's verdicts per hand-built automaton) for one size: computed once, shared, never changed."""
    if n not in _CASES:
        vals = values(n)
        truth = []
        for name, d, closed_form in HAND_BUILT:
            t = np.array([walk(d, v) for v in vals], dtype=bool)
            assert (t == np.array([closed_form(v) for v in vals], dtype=bool)).all(), name   # the automaton is what its name says
            t.setflags(write=False)
            truth.append(t)
        _CASES[n] = (vals, truth)
    return _CASES[n]


# ---- 1. hand-built automata: words, counts, tail bits -----------------------------------------------------------------

@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("n", SIZES)
def test_hand_built_words_and_counts(n, devices):
    vals, truth = case(n)
    with loaded_index(n, devices) as ix:
        base_bool = np.random.default_rng(n + 7).random(n) < 0.6
        if n >= 129:
            base_bool[100] = True
        base = ix.mask(base_bool)
        for pname, parg, pres in present_variants(n, n + 1):
            with ix.text_column(vals, present=parg) as col:
                for bm, bb in ((None, np.ones(n, bool)), (base, base_bool)):
                    for (name, d, _), t in zip(HAND_BUILT, truth):
                        check_mask(col.dfa(d, base=bm), t & pres & bb, (name, pname, bm is not None))
        if n >= 129:   # the verdicts on the 5 KB row: 4998 bytes, no NUL, starts with a, one 0xff
            assert list(t[100] for t in truth) == [True, True, False, True, False, True]


# ---- 2. compiled patterns against Python's `re` -----------------------------------------------------------------------

COMPILED = ["^ab", "ba$", "^$", "a.b", "^[^a]", "é+b", "^.{3}$", "a{3}", "^(a|b)+$", r"\W$", r"\w\W\w", "needle", r"(ab){2,3}", r"\s",
            EMAIL, DOTTED_QUAD]
NEVER = "\udc80-\udcff"   # what bytes that are no UTF-8 decode to below: no `.` and no negated class matches them

_RE_TRUTH = {}


def re_truth(n):
    """Python's verdicts per pattern: the values decoded as UTF-8, every byte that is none as a lone surrogate -- which
    the translated pattern lets no `.`, negated class or negated escape match, as the byte automaton does not."""
    if n not in _RE_TRUTH:
        texts = [v.decode("utf-8", "surrogateescape") for v in values(n)]
        out = {}
        for pattern in COMPILED + ["b.?c"]:
            rx = re.compile(to_python(pattern, NEVER), re.ASCII)
            out[pattern] = np.array([rx.search(t) is not None for t in texts], dtype=bool)
            out[pattern].setflags(write=False)
        _RE_TRUTH[n] = out
    return _RE_TRUTH[n]


@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("n", SIZES)
def test_compiled_patterns(n, devices):
    vals, truth = values(n), re_truth(n)
    with loaded_index(n, devices) as ix:
        rnd = np.random.default_rng(n + 3).random(n) < 0.7
        base_bool = np.random.default_rng(n + 9).random(n) < 0.6
        base = ix.mask(base_bool)
        with ix.text_column(vals) as col, ix.text_column(vals, present=rnd) as some:
            for pattern in COMPILED:
                want = truth[pattern]
                if n >= 777:   # (so the test cannot pass on empty or full masks)
                    assert 3 < int(want.sum()) < n - 3, pattern
                check_mask(col.matches(pattern), want, pattern)
                check_mask(some.matches(pattern, base=base), want & rnd & base_bool, pattern)
            # rows 1 and 2 are b"ab" and b"cd", adjacent in the heap: the state starts again with every row
            if n >= 65:
                assert vals[1] == b"ab" and vals[2] == b"cd"
            assert not truth["b.?c"].any()
            m = col.matches("b.?c")
            assert m.count == 0
            m.close()
            check_mask(col.dfa(regex_dfa.compile("b.?c")), truth["b.?c"])


# ---- 3. the two tiers --------------------------------------------------------------------------------------------------

def test_global_and_lds_tiers():
    n = 1000
    rng = np.random.default_rng(31)
    strings = sorted({bytes(rng.choice(list(b"0123456789abcdef"), 24).tolist()) for _ in range(310)})[:300]
    assert len(strings) == 300
    lds_entries = int(re.search(r"kDfaLdsEntries = (\d+)", open(os.path.join(ROOT, "syzgydb_amd", "csrc", "column_dfa.h")).read()).group(1))
    big, small = regex_dfa.literal_set(strings), regex_dfa.literal_set(strings[:20])
    assert lds_entries == 24576 and big.entries > lds_entries and small.entries <= lds_entries
    assert big.entries <= _lib.SZG_DFA_TABLE_MAX and big.n_states <= _lib.SZG_DFA_STATES_MAX
    vals = values(n)
    order = rng.permutation(300)
    for i, j in enumerate(order[:150]):   # half of the strings are stored; the first 20 among them or not, as it falls
        vals[200 + 5 * i] = strings[j]
    vals[3], vals[4], vals[5] = strings[order[0]][:23], strings[order[0]] + b"0", b"x" + strings[order[0]]   # a prefix, two extensions
    vals[6] = strings[0]
    for dfa, listed in ((big, set(strings)), (small, set(strings[:20]))):
        want = np.array([v in listed for v in vals], dtype=bool)
        assert want.sum() >= 1 and (want == np.array([walk(dfa, v) for v in vals], dtype=bool)).all()
        for devices in (None, [0, 0]):
            with loaded_index(n, devices) as ix, ix.text_column(vals) as col:
                check_mask(col.dfa(dfa), want, (dfa.entries, devices))
                pres = np.random.default_rng(33).random(n) < 0.5
                col.set(6, None)
                base = ix.mask(pres)
                gone = want.copy()
                gone[6] = False
                check_mask(col.dfa(dfa, base=base), gone & pres, (dfa.entries, devices, "base"))
    assert int(np.array([v in set(strings) for v in vals]).sum()) == 151


# ---- 4. refusals on a live column -------------------------------------------------------------------------------------

def raw_dfa(d, **change):
    """(SzgDfa, what keeps its arrays alive) for the raw C call"""
    class_of = np.ascontiguousarray(change.get("class_of", d.class_of), dtype=np.uint8)
    table = np.ascontiguousarray(change.get("next", d.next), dtype=np.uint16)
    bits = np.zeros((d.n_states + 63) // 64, dtype=np.uint64)
    for s in np.flatnonzero(d.accept):
        bits[s // 64] |= np.uint64(1) << np.uint64(s % 64)
    arg = _lib.SzgDfa(change.get("n_states", d.n_states), change.get("n_classes", d.n_classes), change.get("start", d.start),
                      class_of.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                      bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    return arg, (class_of, table, bits)


def test_refusals_on_a_live_column():
    n = 200
    vals = values(n)
    d = regex_dfa.compile("^ab")
    ix, other = loaded_index(n, [0, 0]), loaded_index(n, None)
    try:
        L = ix._L
        text = ix.text_column(vals)
        numbers = ix.column(np.arange(n, dtype=np.float64))
        codes = ix.column(np.arange(n, dtype=np.uint32))
        out = ctypes.c_void_p(0x1234)
        good, keep = raw_dfa(d)
        # a column of another kind
        for c in (numbers, codes):
            assert L.szg_mask_where_dfa(c._h, ctypes.byref(good), None, ctypes.byref(out)) == _lib.SZG_E_INVALID
            assert b"kind does not match" in L.szg_last_error()
            with pytest.raises(SzgError) as e:
                c.dfa(d)
            assert e.value.code == _lib.SZG_E_INVALID
            with pytest.raises(SzgError):
                c.matches("^ab")
        # bad tables: refused by the host's check of the whole table, whatever the column
        bad_next, bad_class = d.next.copy(), d.class_of.copy()
        bad_next[-1, -1] = d.n_states
        bad_class[255] = d.n_classes
        for change in ({"next": bad_next}, {"class_of": bad_class}, {"start": d.n_states}, {"n_classes": 0}, {"n_states": 0}):
            arg, keep2 = raw_dfa(d, **change)
            assert L.szg_mask_where_dfa(text._h, ctypes.byref(arg), None, ctypes.byref(out)) == _lib.SZG_E_INVALID, change
            assert b"dfa" in L.szg_last_error()
        for change in ({"n_states": 32769}, {"n_states": 32768, "n_classes": 256}):
            arg, keep2 = raw_dfa(d, **change)
            assert L.szg_mask_where_dfa(text._h, ctypes.byref(arg), None, ctypes.byref(out)) == _lib.SZG_E_UNSUPPORTED, change
        with pytest.raises(SzgError) as e:
            text.dfa(regex_dfa.Dfa(d.class_of, bad_next, d.accept, 0))
        assert e.value.code == _lib.SZG_E_INVALID and "dfa" in str(e.value)
        with pytest.raises(regex_dfa.DfaTooLarge):
            text.matches("(a|b)*a(a|b){16}")
        with pytest.raises(ValueError):
            text.matches("(?i)a")
        # base masks: closed, of another handle
        closed = ix.mask(np.ones(n, bool))
        closed.close()
        with pytest.raises(ValueError):
            text.dfa(d, base=closed)
        foreign = other.mask(np.ones(n, bool))
        assert L.szg_mask_where_dfa(text._h, ctypes.byref(good), foreign._live(), ctypes.byref(out)) == _lib.SZG_E_INVALID
        with pytest.raises(SzgError) as e:
            text.dfa(d, base=foreign)
        assert e.value.code == _lib.SZG_E_INVALID
        check_mask(text.dfa(d), np.array([v.startswith(b"ab") for v in vals]))   # the column works
        # short: rows appended to the index but not to the column; a stale base
        old = ix.mask(np.ones(n, bool))
        ix.append(orc.synth_rows(SEED + 2, 0, 1, DIM, BITS))
        assert L.szg_mask_where_dfa(text._h, ctypes.byref(good), None, ctypes.byref(out)) == _lib.SZG_E_INVALID
        assert b"short column" in L.szg_last_error()
        text.append([b"abc"])
        with pytest.raises(SzgError) as e:
            text.dfa(d, base=old)
        assert e.value.code == _lib.SZG_E_INVALID and "stale mask" in str(e.value)
        check_mask(text.matches("^ab"), np.array([v.startswith(b"ab") for v in vals + [b"abc"]]))
        # stale: the handle's rows were loaded again
        ix.load(orc.synth_rows(SEED + 1, 0, n, DIM, BITS))
        assert L.szg_mask_where_dfa(text._h, ctypes.byref(good), None, ctypes.byref(out)) == _lib.SZG_E_INVALID
        assert b"stale column" in L.szg_last_error()
        with pytest.raises(SzgError) as e:
            text.matches("^ab")
        assert e.value.code == _lib.SZG_E_INVALID and "stale column" in str(e.value)
        assert out.value == 0x1234
    finally:
        other.close()
        ix.close()


# ---- 5. the Collection ------------------------------------------------------------------------------------------------

email, name, price, other = Field("email"), Field("name"), Field("price"), Field("other")


def collection_metadata(n):
    rng = np.random.default_rng(41)
    users = ["ann", "bob", "é", "a b", "x.y", "", "q@q", "needle"]
    hosts = ["example.org", "b.cd", "€.info", "nodot", "x.museum", "UPPER.ORG", "z.toolongtld"]
    names = ["a", "ab", "abab", "ababab", "b", "needle", "é", ""]
    out = []
    for i in range(n):
        kind = i % 11
        if kind == 0:
            out.append(b"not json")
        elif kind == 1:
            out.append(b'{"email": 5, "name": 7, "price": 1}')
        elif kind == 2:
            out.append(('{"name": "%s", "price": %s}' % (names[rng.integers(len(names))], rng.integers(0, 12) * 0.5)).encode())
        elif kind == 3:
            out.append(b'["someone@example.org"]')
        else:
            out.append(('{"email": "%s@%s", "name": "%s", "price": %s, "other": "%s@b.cd"}'
                        % (users[rng.integers(len(users))], hosts[rng.integers(len(hosts))], names[rng.integers(len(names))],
                           rng.integers(0, 12) * 0.5, users[rng.integers(len(users))])).encode())
    return out


def test_collection_matches_equals_filter():
    n = 300
    metas = collection_metadata(n)
    V = orc.synth_vectors(SEED + 5, 0, n + 10, DIM)
    q = orc.synth_vectors(SEED + 6, 0, 3, DIM)
    same = tgc.assert_same_answers
    c = Collection(CollectionOptions(Name="dfa", DistanceMethod=1, DimensionCount=DIM, Quantization=BITS), devices=[0, 0])
    try:
        c.AddDocuments(range(1000, 1000 + n), V[:n], metas)
        c.IndexField("price", "number")
        c.IndexField("email", "text")
        c.IndexField("name", "string")
        on_text = [email.matches(EMAIL), ~email.matches(EMAIL), email.matches("^ann@") | (price < 2), email.matches(r"\.org$") & (price >= 2),
                   email.matches(""), email.matches("é|€"), ~(email.matches("^$") | email.matches("q@q@"))]
        matched = sum(e.evaluate(m) for e in on_text[:1] for m in metas)
        assert 3 < matched < n - 3   # (the comparison has rows on both sides)
        same(c, q, on_text)
        compiled = c.where_compiled
        assert compiled >= len(on_text) and c.where_fallbacks == 0
        # a "string" field: once per dictionary entry
        on_string = [name.matches("^(ab)+$"), ~name.matches("a"), name.matches("^$") | email.matches("needle")]
        same(c, q, on_string)
        assert c.where_compiled >= compiled + len(on_string) and c.where_fallbacks == 0
        compiled = c.where_compiled
        # a field that is not indexed, and a pattern whose table is beyond the kernel's limits: the host answers
        fallbacks = [other.matches("^ann@"), email.matches(EMAIL) & other.matches("b"), email.matches("(a|b)*a(a|b|n){16}")]
        same(c, q, fallbacks)
        assert c.where_fallbacks >= len(fallbacks) and c.where_compiled == compiled
        # mutations, then a compaction: the carried column serves the automaton
        c.UpdateDocument(1004, b'{"email": "new@example.org", "name": "abab", "price": 1}')
        c.AddDocument(2000, V[n], b'{"email": "late@example.org", "name": "ab", "price": 0.5}')
        assert c.RemoveDocuments([1005, 1016, 1100, 1299]) == 4
        same(c, q, on_text[:3] + on_string[:1])
        assert c.Compact() == 4
        fb = c.where_fallbacks
        same(c, q, on_text + on_string)
        assert c.where_fallbacks == fb
        got = c.Search(SearchArgs(Where=email.matches("^(new|late)@"), Limit=10))
        assert sorted(r.ID for r in got.Results) == [1004, 2000]
    finally:
        c.Close()
