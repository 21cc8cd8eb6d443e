"""MATCHES as a byte automaton, the parts that need no GPU: the pattern compiler (syzgydb_amd/regex_dfa.py) against
Python's `re` -- a fixed list of patterns and 500 seeded random ones over the supported subset, texts with "\\n", NUL and
2-, 3- and 4-byte code points --, the syntax it refuses, the blow-up exception and the lazy walker that answers
anyway, the Matches node of where.py, the C symbol's argument checks (every one precedes device work), and the
stand-alone program that runs the kernel's predicate and the host-side helpers (syzgydb_amd/csrc/column_dfa.h) under
the sanitizers.  test_gpu_text_dfa.py has the device side."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from syzgydb_amd import Field, _lib, regex_dfa
from syzgydb_amd import where as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GO_SPACE = "\\t\\n\\f\\r "


def to_python(pattern, never=""):
    """The pattern for Python's `re` (compiled with re.ASCII, used with search): Go's `$` and \\z are \\Z, Go's \\s and
    \\S are spelled out as their sets -- without brackets inside a class.  never: the body of a class of characters that
    no `.`, negated class or negated escape may match (test_gpu_text_dfa.py: what bytes that are not UTF-8 decode to)."""
    out, i, in_class = [], 0, False
    while i < len(pattern):
        ch = pattern[i]
        if ch == "\\":
            nxt = pattern[i + 1]
            if nxt == "s":
                out.append(GO_SPACE if in_class else "[" + GO_SPACE + "]")
            elif nxt in "SDW":
                assert not in_class, "a negated escape inside a class has no spelling here"
                out.append("[^" + (GO_SPACE if nxt == "S" else "\\" + nxt.lower()) + never + "]")
            elif nxt == "z":
                out.append("\\Z")
            else:
                out.append(ch + nxt)
            i += 2
            continue
        if in_class:
            in_class = ch != "]"
            out.append(ch)
        elif ch == "[":
            in_class = True
            out.append(ch)
            if pattern[i + 1:i + 2] == "^":
                out.append("^" + never)
                i += 1
            if pattern[i + 1:i + 2] == "]":   # a first ] is a literal
                out.append("\\]")
                i += 1
        elif ch == "$":
            out.append("\\Z")
        elif ch == "." and never:
            out.append("[^\\n" + never + "]")
        else:
            out.append(ch)
        i += 1
    return "".join(out)


def python_verdicts(pattern, texts):
    rx = re.compile(to_python(pattern), re.ASCII)
    return [rx.search(t) is not None for t in texts]


EMAIL = r"^[^@\s]+@[^@\s]+\.[a-z]{2,6}$"
DOTTED_QUAD = r"^(\d{1,3}\.){3}\d{1,3}$"

PATTERNS = [
    # anchors at both ends, ^$, the empty pattern, an empty alternative
    "^abc$", "^abc", "abc$", "abc", "^$", "", "a|", "|a", "^a|b$", "(^a|b)$", "$^", r"\Aab\z", "^(a|$)", "a$|^b", "(a|^)b",
    # . against "\n" and 2-, 3- and 4-byte code points; a negated class against the same
    ".", "^.$", "^..$", "a.c", "^.*$", ".*", "^[^a]$", "[^a]", "^[^a\n]$", "^[^é]$", "^[^€]+$", "^[^\U0001F600]$",
    "^[à-ÿ]$", "^[a-€]+$", "^[^a-€]+$", "^[\u0080-\U0010FFFF]$",
    "é+", "^é+$", "(?:é)+€", "€|\U0001F600",
    # counted repeats
    "a{2}", "^a{2}$", "^a{2,}$", "^a{0,2}$", "^(ab){2,3}$", "a{2,3}?b", "(a|b){3}c", "^.{3}$", "^.{2,4}$", "x{0}y", "^(a{2}){2}$",
    "a{", "a{1", "a{1,2",   # (RE2 and Python both read these braces as literals)
    # classes and escapes
    r"\d+", r"^\w+$", r"\s", r"^\S+$", r"\D", r"^\W$", r"[\d.]+", r"[^\s@]+@", r"[\w-]+", r"[]a]", r"[^]a]", r"[a\]]", r"a\.b", r"\^\$",
    r"\n", r"a\tb", r"[\n\t]", r"\\", r"[a-c1-3]+\.", r"\v|\f", r"[-a]", r"[a-]",
    EMAIL, DOTTED_QUAD,
    # groups, alternation, stars
    "(a|b)*abb", "^(a|b)*$", "(?:ab)*c", "(a*)*b", "(a|ab)(c|bcd)", "^(|a)+$", "a*?b", "a+?", "a??b", "(a+)+$", "((a)|(b))+c",
    "(a|b)*a(a|b){7}",
]

ALPHABET = ["a", "b", "c", "@", ".", "1", " ", "\n", "\0", "é", "€", "\U0001F600"]

HAND_TEXTS = ["", "a", "b", "ab", "abc", "abcabc", "xabc", "abcx", "\n", "a\n", "\na", "abc\n", "é", "éé", "€", "\U0001F600", "aé€\U0001F600",
              "a.c", "a\nc", "aéc", "a€c", "a\U0001F600c", "someone@example.org", "some one@example.org", "a@b.c", "a@b.cd",
              "a@b.cdefghi", "@b.cd", "1.2.3.4", "192.168.1.255", "1.2.3", "1.2.3.4.5", "1234.1.1.1", "aab", "abb", "babb", "aaaa",
              "]", "a]", "^$", "\\", "a\tb", "\v", "\f", "\x7f", "ÿ", "Ā", "߿", "ࠀ", "￿", "\U00010000",
              "\U0010FFFF", "퟿", "", "a{", "a{1", "a{1,2", "a{,2}", "a-", "-", "a_b-c", "ab" * 15, "a" * 12]   # (no longer runs of a: Python backtracks on (a*)*b)


def random_texts(rng, count):
    return ["".join(rng.choice(ALPHABET) for _ in range(rng.randrange(0, 31))) for _ in range(count)]


def check_pattern(pattern, texts):
    """Every text: the lazy walker and the full table against Python; returns the number of matches."""
    want = python_verdicts(pattern, texts)
    lazy = regex_dfa.matcher(pattern)
    full = regex_dfa.compile(pattern)
    assert full.start == 0 and full.class_of.shape == (256,) and full.next.shape == (full.n_states, full.n_classes)
    assert int(full.class_of.max()) + 1 == full.n_classes and int(full.next.max()) < full.n_states
    for t, w in zip(texts, want):
        b = t.encode("utf-8")
        assert lazy.match(b) == w, (pattern, t, w)
        assert full.match(b) == w, (pattern, t, w)
    return sum(want)


def test_fixed_patterns_agree_with_python():
    texts = HAND_TEXTS + random_texts(random.Random(1), 300)
    matched = 0
    for pattern in PATTERNS:
        matched += check_pattern(pattern, texts)
    assert 0 < matched < len(PATTERNS) * len(texts)
    # RE2 reads {,2} as a literal as well (Python as {0,2}: not in the list)
    assert regex_dfa.matcher("a{,2}").match(b"xa{,2}") and not regex_dfa.matcher("a{,2}").match(b"aa")
    # what the issue's prototype measured: ordinary patterns sit far inside the kernel's LDS tier
    assert regex_dfa.compile(EMAIL).entries < 4096
    assert regex_dfa.compile("(a|b)*a(a|b){7}").n_states <= 130


# ---- random patterns over the subset ------------------------------------------------------------------------------------
# Python's backtracking matcher must stay quick: the body of an unbounded repeat holds no repeat of its own, and an
# alternation there is one of distinct single letters; counts stay at 3 or less, groups nest once and repeat twice at
# most, which keeps the tables at a few thousand states.

SINGLES = ["a", "b", "c", "@", "1", " ", "é", "€", "\U0001F600", r"\.", r"\n", ".", "[abc]", "[^a]", "[a-c1]", "[^\\n]", r"[\d.]", r"[^\s@]",
           "[^é]", "[b-€]", r"\d", r"\w", r"\s", r"\D", r"\W", r"\S"]


def gen_single(rng):
    return rng.choice(SINGLES)


def gen_plain(rng):
    """A body for an unbounded repeat: single characters in a row, or an alternation of distinct letters."""
    if rng.random() < 0.3:
        return "(" + "|".join(rng.sample(["a", "b", "c", "é", "1"], rng.randrange(2, 4))) + ")"
    items = [gen_single(rng) for _ in range(rng.randrange(1, 3))]
    return items[0] if len(items) == 1 else "(?:" + "".join(items) + ")"


def gen_item(rng, depth):
    roll = rng.random()
    if roll < 0.25:   # an unbounded repeat
        op = rng.choice(["*", "+", "{1,}", "{2,}", "*?", "+?"])
        return gen_plain(rng) + op
    if depth > 0 and roll < 0.45:   # a group, perhaps with a bounded repeat
        body = gen_alt(rng, depth - 1)
        group = rng.choice(["(%s)", "(?:%s)"]) % body
        return group + rng.choice(["", "", "?", "{2}", "{0,2}", "??"])
    single = gen_single(rng)
    return single + rng.choice(["", "", "", "?", "{2}", "{3}", "{0,2}", "{1,2}", "{2}?"])


def gen_cat(rng, depth):
    return "".join(gen_item(rng, depth) for _ in range(rng.randrange(1, 4)))


def gen_alt(rng, depth):
    branches = [gen_cat(rng, depth) for _ in range(rng.choice([1, 1, 1, 2, 3]))]
    if rng.random() < 0.1:
        branches.append("")
    return "|".join(branches)


def gen_pattern(rng):
    p = gen_alt(rng, 1)
    if rng.random() < 0.35:
        p = "^" + (p if "|" not in p or rng.random() < 0.5 else "(?:%s)" % p)
    if rng.random() < 0.35:
        p = (p if "|" not in p or rng.random() < 0.5 else "(?:%s)" % p) + rng.choice(["$", r"\z"])
    return p


def test_random_patterns_agree_with_python():
    rng = random.Random(20240)
    patterns = [gen_pattern(rng) for _ in range(500)]
    assert len(set(patterns)) > 450
    shared = ["", "a", "\n", "é", "abc", "a.b@c 1"]
    matched = total = 0
    for pattern in patterns:
        texts = shared + random_texts(rng, 40)
        matched += check_pattern(pattern, texts)
        total += len(texts)
    assert total // 20 < matched < total - total // 20   # (both verdicts are common: the comparison has something to compare)


# ---- refusals and the blow-up ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", ["(?i)a", r"\bx", r"\pL", "(?=a)", r"\1", "a{1001}", "(", "[a",
                                     # and more of what RE2 rejects or the subset leaves out
                                     ")", "a**", "*a", "a{2,1}", "[b-a]", "\\", r"\x41", r"\Qa\E", "(?P<n>a)", "[[:alpha:]]", r"\Z",
                                     "(a{30}){40}", r"[a-\d]", "x{2}{3}", r"\B", r"\C", r"\012"])
def test_rejected_syntax_raises_value_error(pattern):
    with pytest.raises(ValueError):
        regex_dfa.compile(pattern)
    with pytest.raises(ValueError):
        regex_dfa.matcher(pattern)
    with pytest.raises(ValueError):
        Field("f").matches(pattern)


def test_blow_up_raises_and_the_lazy_walker_still_answers():
    pattern = "(a|b)*a(a|b){16}"
    assert not issubclass(regex_dfa.DfaTooLarge, ValueError)
    with pytest.raises(regex_dfa.DfaTooLarge):
        regex_dfa.compile(pattern)
    e = Field("f").matches(pattern)   # building the expression compiles no table
    rng = random.Random(3)
    texts = ["".join(rng.choice("ab") for _ in range(rng.randrange(10, 30))) for _ in range(50)] + ["a" + "b" * 16, "b" + "a" * 16, "c"]
    want = python_verdicts(pattern, texts)
    assert 0 < sum(want) < len(texts)
    for t, w in zip(texts, want):
        assert e.evaluate(('{"f": "%s"}' % t).encode()) == w, t
    # the limits themselves: 32768 states pass, one more does not; the table's entries likewise
    assert (regex_dfa.STATES_MAX, regex_dfa.TABLE_MAX) == (_lib.SZG_DFA_STATES_MAX, _lib.SZG_DFA_TABLE_MAX) == (32768, 1 << 20)
    with pytest.raises(regex_dfa.DfaTooLarge):
        regex_dfa.literal_set([bytes([65 + i % 26, 65 + i // 26 % 26, 65 + i // 676]) * 3 for i in range(6000)])


def test_literal_set_accepts_exactly_its_strings():
    rng = random.Random(4)
    strings = [bytes(rng.choice(b"0123456789abcdef") for _ in range(rng.randrange(0, 9))) for _ in range(200)] + [b"\x00\xff", b"ab"]
    d = regex_dfa.literal_set(strings)
    inside = set(strings)
    assert d.n_classes == 19 and d.start == 0   # 16 digits, NUL, 0xff and the bytes no string holds (a and b are digits)
    for s in strings:
        assert d.match(s)
    for _ in range(2000):
        s = bytes(rng.choice(b"0123456789abcdefg\x00\xff") for _ in range(rng.randrange(0, 10)))
        assert d.match(s) == (s in inside), s
    assert not regex_dfa.literal_set([]).match(b"") and regex_dfa.literal_set([b""]).match(b"")
    every = regex_dfa.literal_set([bytes([b]) for b in range(256)])
    assert every.n_classes == 256 and all(every.match(bytes([b])) for b in range(256)) and not every.match(b"ab")


# ---- where.py ---------------------------------------------------------------------------------------------------------

def test_matches_text_parse_round_trip():
    for pattern in PATTERNS + ['say "hi"', "tab\there", "it's", "back\\\\slash", "new\nline"]:
        e = Field("email").matches(pattern)
        assert isinstance(e, W.Matches) and e.fields() == {"email"}
        text = e.text()
        assert text.startswith("email MATCHES \"")
        back = W.parse(text)
        assert isinstance(back, W.Matches) and back.field == "email" and back.pattern == pattern, pattern
        assert back.text() == text
    both = (Field("a").matches("^x") & ~Field("b").matches("y$")) | (Field("c") < 5)
    assert both.text() == '((a MATCHES "^x" AND NOT (b MATCHES "y$")) OR c < 5)'
    assert W.parse(both.text()).text() == both.text() and both.fields() == {"a", "b", "c"}
    with pytest.raises(TypeError):
        Field("a").matches(5)
    with pytest.raises(ValueError):
        W.parse("a MATCHES 5")
    with pytest.raises(ValueError):
        W.parse('a MATCHES "("')
    assert W.parse("MATCHES2 == 1").fields() == {"MATCHES2"}   # (a longer identifier is no keyword)


def test_matches_evaluate_and_the_error_rule():
    e = Field("email").matches(EMAIL)
    assert e.evaluate(b'{"email": "someone@example.org"}') is True
    assert e.evaluate(b'{"email": "someone@example"}') is False
    assert e.evaluate('{"email": "é@€.org"}'.encode()) is True
    assert Field("n").matches("").evaluate(b'{"n": ""}') is True
    always = Field("other").contains("")   # true wherever `other` is a string
    # an absent field, a number, null, a list: MATCHES needs two strings -- an error, which fails the row ...
    for meta in (b'{"other": "x"}', b'{"email": 5, "other": "x"}', b'{"email": null, "other": "x"}', b'{"email": ["a@b.cd"], "other": "x"}',
                 b'{"email": true, "other": "x"}'):
        assert always.evaluate(meta) is True
        assert e.evaluate(meta) is False
        assert (~e).evaluate(meta) is False          # ... under NOT as well
        assert (always | e).evaluate(meta) is False  # ... and beside a true OR operand
        assert (e | always).evaluate(meta) is False
        with pytest.raises(W._Error):
            e.test(W._value(W.parse_metadata(meta), "email"))
    # metadata that is not a JSON object
    for meta in (b"", b"not json", b"[1]", b'"someone@example.org"', b"5"):
        assert e.evaluate(meta) is False and (~e).evaluate(meta) is False
    # a string that does not match is no error
    meta = b'{"email": "nobody", "other": "x"}'
    assert e.evaluate(meta) is False and (~e).evaluate(meta) is True and (always | e).evaluate(meta) is True


# ---- the C ABI, without a device ------------------------------------------------------------------------------------------

def make_dfa(n_states, n_classes, start, class_of=None, table=None, accept=None):
    """(SzgDfa, what keeps its arrays alive)"""
    cls = (ctypes.c_uint8 * 256)(*(class_of if class_of is not None else [0] * 256))
    nxt = (ctypes.c_uint16 * max(len(table) if table is not None else 4, 1))(*(table if table is not None else [0] * 4))
    acc = (ctypes.c_uint64 * 4)(*(accept if accept is not None else [0] * 4))
    return _lib.SzgDfa(n_states, n_classes, start, cls, nxt, acc), (cls, nxt, acc)


def test_symbol_and_constants():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "syzgy_scan.h")).read()
    assert hasattr(L, "szg_mask_where_dfa") and "szg_mask_where_dfa" in _lib.EXPORTS
    assert re.search(r"\bszg_mask_where_dfa\s*\(", hdr)
    assert re.search(r"#define SZG_DFA_STATES_MAX 32768u", hdr) and re.search(r"#define SZG_DFA_TABLE_MAX\s+\(1u << 20\)", hdr)
    assert (_lib.SZG_DFA_STATES_MAX, _lib.SZG_DFA_TABLE_MAX) == (32768, 1 << 20)
    assert L.szg_abi_version() == 4
    # the struct as the header lays it out: three uint32, then three pointers
    assert ctypes.sizeof(_lib.SzgDfa) == 40 and _lib.SzgDfa.class_of.offset == 16 and _lib.SzgDfa.accept_bits.offset == 32


def test_dfa_arguments_are_checked_on_the_host():
    """Every check precedes device work: these calls run on a machine without a GPU, and *out stays untouched."""
    L = _lib.load()
    out = ctypes.c_void_p(0x1234)
    call = lambda d: L.szg_mask_where_dfa(None, ctypes.byref(d) if d is not None else None, None, ctypes.byref(out))  # noqa: E731
    good, keep = make_dfa(2, 2, 0, [0, 1] * 128, [0, 1, 1, 0], [2])
    assert call(good) == _lib.SZG_E_INVALID and b"null" in L.szg_last_error()   # (the column)
    assert L.szg_mask_where_dfa(None, ctypes.byref(good), None, None) == _lib.SZG_E_INVALID
    assert call(None) == _lib.SZG_E_INVALID and b"null" in L.szg_last_error()
    for name in ("class_of", "next", "accept_bits"):
        d, keep2 = make_dfa(2, 2, 0, [0, 1] * 128, [0, 1, 1, 0], [2])
        setattr(d, name, None)
        assert call(d) == _lib.SZG_E_INVALID and b"null" in L.szg_last_error(), name
    # counts, start, class_of and next entries out of range: "dfa"
    bad = [make_dfa(0, 2, 0), make_dfa(2, 0, 0), make_dfa(2, 257, 0), make_dfa(2, 2, 2), make_dfa(2, 2, 0xFFFFFFFF),
           make_dfa(2, 2, 0, [0] * 255 + [2]), make_dfa(2, 2, 0, [2] + [0] * 255), make_dfa(2, 2, 0, None, [0, 1, 1, 2]),
           make_dfa(2, 2, 0, None, [0xFFFF, 0, 0, 0]), make_dfa(1, 1, 0, None, [1])]
    for d, _ in bad:
        assert call(d) == _lib.SZG_E_INVALID and b"dfa" in L.szg_last_error(), (d.n_states, d.n_classes, d.start)
    # beyond the limits: refused by the counts alone (these tables do not exist)
    for n_states, n_classes in ((32769, 1), (4097, 256), (32768, 33), (0xFFFFFFFF, 256), (1 << 20, 2)):
        d, _ = make_dfa(n_states, n_classes, 0)
        assert call(d) == _lib.SZG_E_UNSUPPORTED and b"dfa" in L.szg_last_error(), (n_states, n_classes)
    assert out.value == 0x1234


def test_standalone_dfa_program_is_clean_under_sanitizers(tmp_path):
    """The walk the kernel runs and the host-side helpers (column_dfa.h), in a stand-alone program with its own main,
    plain g++: hand-built and random automata over values of length 0..17, 255..257 and 5000 at all 16 alignments of a
    heap allocated exactly as the library sizes it, the tables read from an image of exactly the staged size, against a
    bytewise walk; no dword without a byte of the row is fetched, and none behind an absorbing state but the next."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_column_dfa.cpp"
    exe = str(tmp_path / "test_column_dfa")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_column_dfa.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "column dfa ok" in done.stdout


def test_scan_column_dfa_takes_the_compiled_tables():
    """What ScanColumn.dfa hands to the library for a compiled pattern passes the library's own validation: with no
    column the call gets as far as the null check, not a "dfa" refusal."""
    L = _lib.load()
    d = regex_dfa.compile(EMAIL)
    bits = np.zeros((d.n_states + 63) // 64, dtype=np.uint64)
    for s in np.flatnonzero(d.accept):
        bits[s // 64] |= np.uint64(1) << np.uint64(s % 64)
    arg = _lib.SzgDfa(d.n_states, d.n_classes, d.start, d.class_of.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                      d.next.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    out = ctypes.c_void_p(0x1234)
    assert L.szg_mask_where_dfa(None, ctypes.byref(arg), None, ctypes.byref(out)) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error() and out.value == 0x1234
