"""Regular expressions compiled to the byte automata of szg_mask_where_dfa (include/syzgy_scan.h): the host owns the
pattern language, the card walks a table over each row's bytes.

    from syzgydb_amd import regex_dfa
    d = regex_dfa.compile(r"^[^@\\s]+@[^@\\s]+\\.[a-z]{2,6}$")     # a Dfa: class_of, next, accept, start
    d.match(b"someone@example.org")                              # True -- the host walker over the same table
    column.dfa(d)                                                # the same verdicts for every row, on the card
    regex_dfa.matcher(r"(a|b)*a(a|b){16}").match(b"abba")        # a lazy walker: works where the table would not fit
    regex_dfa.literal_set([b"alpha", b"beta"])                   # a Dfa that accepts exactly the listed strings

Semantics: Go's regexp.MatchString (RE2 syntax, no flags set) -- what the reference's MATCHES evaluates
(query/compiler.go:420-431) -- as an UNANCHORED search over the text's UTF-8 bytes.
  * `.` and negated classes are expanded into UTF-8 byte-range sequences: every code point but the surrogates, `.`
    without "\\n".  Bytes that are not valid UTF-8 are matched by no `.` and no class (Go would read each as U+FFFD);
    metadata strings, which come out of a JSON parser, hold none.
  * `^` and `\\A` hold at the start of the text only, `$` and `\\z` at its end only (not before a trailing newline).
  * `\\d \\w \\s` are ASCII sets, `\\s` = [\\t\\n\\f\\r ] (no \\v, unlike Python).
The supported subset: literals, escaped punctuation, \\n \\t \\r \\f \\v; `.`; [...] with ranges, negation and
\\d \\w \\s \\D \\W \\S inside; \\d \\w \\s \\D \\W \\S; ( ), (?: ), |; * + ? {m} {m,} {m,n} with counts <= 1000 (RE2's
limit), each with an optional lazy `?`, which cannot change a yes/no verdict.  Everything else -- flags such as (?i),
\\b \\B, \\p{..}, \\x, octal escapes, \\Q..\\E, [[:alpha:]], named groups -- and everything RE2 itself rejects raises
ValueError when the pattern is compiled.

Construction: a Thompson NFA over bytes with assertion edges -- `^` edges are followed only in the closure of the
initial state, `$` edges only when deciding whether a state set accepts -- determinised by subsets over byte
equivalence classes.  The search is unanchored: the NFA's start is added again after every byte; a set that holds the
NFA's accept state without needing `$` collapses into ONE absorbing accept state, and a set with nothing left that could
still match is the empty set, an absorbing reject -- the two states at which the card stops reading a row.  The table
is built lazily and memoised, so `matcher(p).match` works for every pattern of the subset; `compile` expands it in
full and raises DfaTooLarge past SZG_DFA_STATES_MAX states or SZG_DFA_TABLE_MAX entries.  No minimisation.
"""
import numpy as np

__all__ = ["Dfa", "DfaTooLarge", "Matcher", "compile", "matcher", "literal_set", "STATES_MAX", "TABLE_MAX"]

STATES_MAX = 32768      # SZG_DFA_STATES_MAX
TABLE_MAX = 1 << 20     # SZG_DFA_TABLE_MAX
_REPEAT_MAX = 1000      # RE2's limit on a counted repeat, nested ones multiplied
_MAX_RUNE = 0x10FFFF


class DfaTooLarge(Exception):
    """The pattern's full table exceeds the limits of szg_mask_where_dfa; matcher(pattern).match still answers."""


class Dfa:
    """A complete byte automaton: class_of uint8[256], next uint16[n_states, n_classes], accept bool[n_states], start."""

    def __init__(self, class_of, next, accept, start):
        self.class_of = np.ascontiguousarray(class_of, dtype=np.uint8).reshape(256)
        self.next = np.ascontiguousarray(next, dtype=np.uint16)
        self.accept = np.ascontiguousarray(accept, dtype=bool).reshape(-1)
        self.start = int(start)
        if self.next.ndim != 2 or self.next.shape[0] != self.accept.size:
            raise ValueError("next is [n_states, n_classes], accept [n_states]")

    @property
    def n_states(self):
        return self.next.shape[0]

    @property
    def n_classes(self):
        return self.next.shape[1]

    @property
    def entries(self):
        return self.next.size

    def match(self, data):
        """The verdict on one byte string: the state after every byte, from start, accepts."""
        s, nxt, cls = self.start, self.next, self.class_of
        for b in bytes(data):
            s = nxt[s, cls[b]]
        return bool(self.accept[s])


# ---- pattern text -> tree ---------------------------------------------------------------------------------------------
# nodes: ("empty",) ("set", [(lo, hi) code point ranges, sorted, disjoint]) ("bol",) ("eol",) ("cat", [nodes])
#        ("alt", [nodes]) ("rep", node, m, n or None)

_DIGIT = [(0x30, 0x39)]
_WORD = [(0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A)]
_SPACE = [(0x09, 0x0A), (0x0C, 0x0D), (0x20, 0x20)]
_PERL = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
_CONTROL = {"n": 0x0A, "t": 0x09, "r": 0x0D, "f": 0x0C, "v": 0x0B}


def _normalise(ranges):
    out = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def _negate(ranges):
    out, at = [], 0
    for lo, hi in _normalise(ranges):
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= _MAX_RUNE:
        out.append((at, _MAX_RUNE))
    return out


class _Parser:
    def __init__(self, pattern):
        if not isinstance(pattern, str):
            raise TypeError("a pattern is a str")
        for ch in pattern:
            if 0xD800 <= ord(ch) <= 0xDFFF:
                raise ValueError("pattern: a surrogate is not a character")
        self.p, self.i = pattern, 0

    def error(self, what):
        return ValueError("pattern %r: %s at %d" % (self.p, what, self.i))

    def more(self):
        return self.i < len(self.p)

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alternation()
        if self.more():
            raise self.error("unexpected )")
        _check_repeats(node, 1, self)
        return node

    def alternation(self):
        branches = [self.concatenation()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.concatenation())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def concatenation(self):
        items = []
        while self.more() and self.peek() not in "|)":
            items.append(self.repeat(self.atom()))
        if not items:
            return ("empty",)
        return items[0] if len(items) == 1 else ("cat", items)

    def repeat(self, node):
        repeated = False
        while self.more():
            ch = self.peek()
            if ch == "*":
                m, n, width = 0, None, 1
            elif ch == "+":
                m, n, width = 1, None, 1
            elif ch == "?":
                m, n, width = 0, 1, 1
            elif ch == "{":
                counted = self.counted()
                if counted is None:
                    return node   # (RE2: a { that opens no repeat is a literal; the caller reads it as one)
                m, n, width = counted
            else:
                return node
            if repeated:
                raise self.error("invalid nested repetition operator")
            self.i += width
            if self.peek() == "?":   # lazy: the same verdict
                self.i += 1
            if m > _REPEAT_MAX or (n is not None and (n > _REPEAT_MAX or n < m)):
                raise self.error("bad repetition count")
            node = ("rep", node, m, n)
            repeated = True
        return node

    def counted(self):
        """(m, n, characters) of a {m} {m,} {m,n} at the cursor, or None when the brace opens no repeat."""
        j = self.i + 1
        k = j
        while k < len(self.p) and self.p[k].isascii() and self.p[k].isdigit():
            k += 1
        if k == j:
            return None
        m, n = int(self.p[j:k]), None
        if k < len(self.p) and self.p[k] == ",":
            k += 1
            j = k
            while k < len(self.p) and self.p[k].isascii() and self.p[k].isdigit():
                k += 1
            if k > j:
                n = int(self.p[j:k])
        else:
            n = m
        if k >= len(self.p) or self.p[k] != "}":
            return None
        return m, n, k + 1 - self.i

    def atom(self):
        ch = self.p[self.i]
        if ch in "*+?":
            raise self.error("missing argument to repetition operator")
        if ch == "(":
            self.i += 1
            if self.peek() == "?":
                if self.p[self.i:self.i + 2] != "?:":
                    raise self.error("flags, named groups and look-around are outside the supported subset")
                self.i += 2
            node = self.alternation()
            if self.peek() != ")":
                raise self.error("missing )")
            self.i += 1
            return node
        if ch == "[":
            return self.char_class()
        if ch == ".":
            self.i += 1
            return ("set", _negate([(0x0A, 0x0A)]))
        if ch == "^":
            self.i += 1
            return ("bol",)
        if ch == "$":
            self.i += 1
            return ("eol",)
        if ch == "\\":
            return self.escape()
        self.i += 1
        return ("set", [(ord(ch), ord(ch))])

    def escape_char(self):
        """The code point of the escaped character after the backslash at the cursor, or None for another escape."""
        if self.i + 1 >= len(self.p):
            raise self.error("trailing backslash")
        ch = self.p[self.i + 1]
        if ch in _CONTROL:
            self.i += 2
            return _CONTROL[ch]
        if ch.isascii() and not ch.isalnum():   # (RE2: any ASCII character that is neither a letter nor a digit)
            self.i += 2
            return ord(ch)
        return None

    def escape(self):
        c = self.escape_char()
        if c is not None:
            return ("set", [(c, c)])
        ch = self.p[self.i + 1]
        if ch in "dws":
            self.i += 2
            return ("set", list(_PERL[ch]))
        if ch in "DWS":
            self.i += 2
            return ("set", _negate(_PERL[ch.lower()]))
        if ch == "A":
            self.i += 2
            return ("bol",)
        if ch == "z":
            self.i += 2
            return ("eol",)
        raise self.error("the escape \\%s is outside the supported subset" % ch)

    def class_char(self):
        if not self.more():
            raise self.error("missing ]")
        if self.peek() == "\\":
            c = self.escape_char()
            if c is None:
                raise self.error("the escape \\%s cannot stand here" % self.p[self.i + 1])
            return c
        self.i += 1
        return ord(self.p[self.i - 1])

    def char_class(self):
        self.i += 1
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        ranges, first = [], True
        while True:
            if not self.more():
                raise self.error("missing ]")
            if self.peek() == "]" and not first:
                self.i += 1
                break
            first = False
            if self.p[self.i:self.i + 2] == "[:":
                raise self.error("[:name:] classes are outside the supported subset")
            if self.peek() == "\\" and self.i + 1 < len(self.p) and self.p[self.i + 1] in "dwsDWS":
                ch = self.p[self.i + 1]
                ranges += _PERL[ch] if ch in "dws" else _negate(_PERL[ch.lower()])
                self.i += 2
                continue
            lo = hi = self.class_char()
            if self.peek() == "-" and self.i + 1 < len(self.p) and self.p[self.i + 1] != "]":
                self.i += 1
                hi = self.class_char()
                if hi < lo:
                    raise self.error("bad character class range")
            ranges.append((lo, hi))
        ranges = _normalise(ranges)
        return ("set", _negate(ranges) if negate else ranges)


def _check_repeats(node, product, parser):
    """RE2 refuses counted repeats whose nested counts multiply past 1000."""
    kind = node[0]
    if kind == "rep":
        count = max(node[2], node[3] or 0)
        if count > 1:
            product *= count
            if product > _REPEAT_MAX:
                raise ValueError("pattern %r: nested repetition counts exceed %d" % (parser.p, _REPEAT_MAX))
        _check_repeats(node[1], product, parser)
    elif kind in ("cat", "alt"):
        for child in node[1]:
            _check_repeats(child, product, parser)


# ---- code point ranges -> UTF-8 byte-range sequences ------------------------------------------------------------------

def _encode(c):
    if c <= 0x7F:
        return [c]
    if c <= 0x7FF:
        return [0xC0 | (c >> 6), 0x80 | (c & 0x3F)]
    if c <= 0xFFFF:
        return [0xE0 | (c >> 12), 0x80 | ((c >> 6) & 0x3F), 0x80 | (c & 0x3F)]
    return [0xF0 | (c >> 18), 0x80 | ((c >> 12) & 0x3F), 0x80 | ((c >> 6) & 0x3F), 0x80 | (c & 0x3F)]


def _utf8_sequences(lo, hi):
    """[lo, hi] of code points as sequences of byte ranges [(b_lo, b_hi), ...]: together they match exactly the UTF-8
    encodings of the range's code points, the surrogates left out."""
    out, stack = [], [(lo, hi)]
    while stack:
        lo, hi = stack.pop()
        if lo > hi:
            continue
        if lo <= 0xDFFF and hi >= 0xD800:
            stack += [(lo, 0xD7FF), (0xE000, hi)]
            continue
        for edge in (0x7F, 0x7FF, 0xFFFF):   # one encoded length per piece
            if lo <= edge < hi:
                stack += [(lo, edge), (edge + 1, hi)]
                break
        else:
            if hi <= 0x7F:
                out.append([(lo, hi)])
                continue
            for i in (1, 2, 3):   # the continuation bytes behind a differing byte must span their whole range
                m = (1 << (6 * i)) - 1
                if (lo & ~m) != (hi & ~m):
                    if lo & m:
                        stack += [(lo, lo | m), ((lo | m) + 1, hi)]
                        break
                    if (hi & m) != m:
                        stack += [(lo, (hi & ~m) - 1), (hi & ~m, hi)]
                        break
            else:
                out.append(list(zip(_encode(lo), _encode(hi))))
    return out


# ---- tree -> NFA -------------------------------------------------------------------------------------------------------

class _Nfa:
    def __init__(self):
        self.bytes = []   # per state: [(lo, hi, target)]
        self.eps = []     # per state: [target]
        self.bol = []     # per state: [target], followed at the start of the text only
        self.eol = []     # per state: [target], followed at the end of the text only

    def state(self):
        for edges in (self.bytes, self.eps, self.bol, self.eol):
            edges.append([])
        return len(self.eps) - 1

    def build(self, node):
        """(entry, exit) of the fragment for `node`."""
        kind = node[0]
        a, b = self.state(), self.state()
        if kind == "empty":
            self.eps[a].append(b)
        elif kind == "bol":
            self.bol[a].append(b)
        elif kind == "eol":
            self.eol[a].append(b)
        elif kind == "set":
            for lo, hi in node[1]:
                for seq in _utf8_sequences(lo, hi):
                    at = a
                    for j, (blo, bhi) in enumerate(seq):
                        to = b if j == len(seq) - 1 else self.state()
                        self.bytes[at].append((blo, bhi, to))
                        at = to
        elif kind == "cat":
            at = a
            for child in node[1]:
                ca, cb = self.build(child)
                self.eps[at].append(ca)
                at = cb
            self.eps[at].append(b)
        elif kind == "alt":
            for child in node[1]:
                ca, cb = self.build(child)
                self.eps[a].append(ca)
                self.eps[cb].append(b)
        else:
            _, child, m, n = node
            at = a
            for _ in range(m):
                ca, cb = self.build(child)
                self.eps[at].append(ca)
                at = cb
            if n is None:      # child*
                ca, cb = self.build(child)
                loop = self.state()
                self.eps[at].append(loop)
                self.eps[loop] += [ca, b]
                self.eps[cb].append(loop)
            else:              # (child(child(...)?)?)?
                for _ in range(n - m):
                    ca, cb = self.build(child)
                    self.eps[at] += [ca, b]
                    at = cb
                self.eps[at].append(b)
        return a, b


# ---- NFA -> DFA, lazily -------------------------------------------------------------------------------------------------

_MATCH = "match"   # the key of the absorbing accept state


class Matcher:
    """A compiled pattern as a lazily determinised automaton: match(bytes) builds the states a text visits, dfa() all."""

    def __init__(self, pattern):
        self.pattern = pattern
        nfa = self._nfa = _Nfa()
        self._first, self._last = nfa.build(_Parser(pattern).parse())
        # byte equivalence classes: the bytes between two neighbouring edge boundaries move every state alike
        cut = np.zeros(257, dtype=bool)
        cut[0] = True
        for edges in nfa.bytes:
            for lo, hi, _ in edges:
                cut[lo] = cut[hi + 1] = True
        self.class_of = (np.cumsum(cut[:256]) - 1).astype(np.uint8)
        self.n_classes = int(self.class_of[255]) + 1
        self._sample = [int(np.argmax(self.class_of == c)) for c in range(self.n_classes)]   # a byte of each class
        self._class_list = self.class_of.tolist()
        self._ids, self._keys, self._rows, self._accept = {}, [], [], []
        self._important = [bool(nfa.bytes[s] or nfa.eol[s]) or s == self._last for s in range(len(nfa.eps))]
        self._has_bol = any(nfa.bol)   # (without a `^` the initial state is a state like any other)
        self._reach, self._moves = {}, {}
        self._restart = self._kept(self._closure([self._first], False))   # what every byte adds: the search is unanchored
        self._state(self._kept(self._closure([self._first], True)), True)

    def _closure(self, seeds, at_start, at_end=False):
        """Every state reachable from the seeds without a byte: `^` edges only at the start, `$` edges only at the end."""
        nfa, seen, stack = self._nfa, set(seeds), list(seeds)
        while stack:
            s = stack.pop()
            for t in nfa.eps[s]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
            for edges, on in ((nfa.bol[s], at_start), (nfa.eol[s], at_end)):
                if on:
                    for t in edges:
                        if t not in seen:
                            seen.add(t)
                            stack.append(t)
        return seen

    def _kept(self, closed):
        """Only the states with something ahead of them -- a byte edge, a `$` edge, the accept state -- tell two closed
        sets apart."""
        return frozenset(s for s in closed if self._important[s])

    def _move(self, s):
        """[(byte class, the kept closure of what NFA state s reaches on a byte of the class)], classes that lead
        nowhere left out."""
        row = self._moves.get(s)
        if row is None:
            row = []
            for c, b in enumerate(self._sample):
                out = set()
                for lo, hi, to in self._nfa.bytes[s]:
                    if lo <= b <= hi:
                        reach = self._reach.get(to)
                        if reach is None:
                            reach = self._reach[to] = self._kept(self._closure([to], False))
                        out |= reach
                if out:
                    row.append((c, out))
            self._moves[s] = row
        return row

    def _state(self, kept, initial=False):
        """The number of the automaton's state for a kept closed set of NFA states."""
        key = _MATCH if self._last in kept else (kept, initial and self._has_bol)
        n = self._ids.get(key)
        if n is None:
            n = self._ids[key] = len(self._keys)
            self._keys.append(key)
            self._rows.append(None)
            if key == _MATCH:
                self._accept.append(True)
            else:   # at the end of the text: `$` holds, `^` only if nothing was read
                self._accept.append(self._last in self._closure(kept, key[1], True))
        return n

    def _step(self, n, c):
        row = self._rows[n]
        if row is None:   # the whole row at the first visit: one pass over the set's NFA states
            key = self._keys[n]
            if key == _MATCH:
                row = [n] * self.n_classes
            else:
                moved = [None] * self.n_classes
                for s in key[0]:
                    for cls, reach in self._move(s):
                        if moved[cls] is None:
                            moved[cls] = set(reach)
                        else:
                            moved[cls] |= reach
                row = [self._state(self._restart if m is None else frozenset(m | self._restart)) for m in moved]
            self._rows[n] = row
        return row[c]

    def match(self, data):
        """Go's regexp.MatchString(pattern, text) for the text's UTF-8 bytes."""
        n, cls = 0, self._class_list
        for b in bytes(data):
            n = self._step(n, cls[b])
            if self._keys[n] == _MATCH:
                return True
        return self._accept[n]

    def dfa(self):
        """The whole table as a Dfa (state 0 is the start); DfaTooLarge past the limits of szg_mask_where_dfa."""
        n = 0
        while n < len(self._keys):
            if len(self._keys) > STATES_MAX or len(self._keys) * self.n_classes > TABLE_MAX:   # (also when asked again)
                raise DfaTooLarge("pattern %r: more than %d states or %d table entries"
                                  % (self.pattern, STATES_MAX, TABLE_MAX))
            self._step(n, 0)
            n += 1
        return Dfa(self.class_of, np.array(self._rows, dtype=np.uint16).reshape(len(self._keys), self.n_classes),
                   np.array(self._accept, dtype=bool), 0)


def matcher(pattern):
    """The pattern as a Matcher; ValueError for syntax outside the supported subset."""
    return Matcher(pattern)


def compile(pattern):
    """The pattern's complete Dfa; ValueError for syntax outside the subset, DfaTooLarge for a table beyond the limits."""
    return Matcher(pattern).dfa()


def literal_set(strings):
    """A Dfa that accepts exactly the listed byte strings (a trie: one state per distinct prefix, and a dead state)."""
    strings = [bytes(s) for s in strings]
    used = sorted({b for s in strings for b in s})
    class_of = np.zeros(256, dtype=np.uint8)   # class 0: the bytes no string holds
    n_classes = len(used) + 1
    if n_classes > 256:   # every byte value occurs: no class of unused bytes
        n_classes = 256
        class_of[:] = np.arange(256, dtype=np.uint8)
    else:
        for i, b in enumerate(used):
            class_of[b] = i + 1
    rows, accept = [[1] * n_classes, [1] * n_classes], [False, False]   # state 0: the root; state 1: dead
    for s in strings:
        at = 0
        for b in s:
            c = int(class_of[b])
            if rows[at][c] == 1:
                if len(rows) >= STATES_MAX or (len(rows) + 1) * n_classes > TABLE_MAX:
                    raise DfaTooLarge("literal_set: more than %d states or %d table entries" % (STATES_MAX, TABLE_MAX))
                rows[at][c] = len(rows)
                rows.append([1] * n_classes)
                accept.append(False)
            at = rows[at][c]
        accept[at] = True
    return Dfa(class_of, np.array(rows, dtype=np.uint16), np.array(accept, dtype=bool), 0)
