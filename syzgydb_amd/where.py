"""A small expression tree over top-level metadata fields, in the reference's filter language.

    from syzgydb_amd.where import Field
    e = (Field("price") < 37.5) & ~Field("brand").isin(["acme", "apex"])
    e.text()        # '(price < 37.5 AND NOT (brand IN ["acme", "apex"]))' -- the same filter for a Go or REST caller
    e.fields()      # {"price", "brand"}
    e.evaluate(b'{"price": 12, "brand": "zeta"}')   # True

Collection.Search(SearchArgs(Where=e)) compiles such a tree to a filter mask on the card through the collection's
indexed fields (Collection.IndexField); `evaluate` is the host evaluator -- the fallback for fields that are not
indexed, and the yardstick the device path is tested against.  It restates the reference's rules:

  * Metadata that is not valid JSON, or not a JSON object, fails the filter: json.Unmarshal's error, or getField's
    "cannot access field" on a non-map, becomes `false` (query/compiler.go:477-497, :433-447; collection.go:203-218).
  * An absent field is nil (a Go map lookup, compiler.go:438), and so is a JSON null.
  * `==` is reflect.DeepEqual (compiler.go:175): a number field equals a number constant by float64 ==
    (so -0.0 == 0), a string field equals a string constant by its bytes, everything else -- nil, bools, arrays,
    objects, a number against a string -- is false.  `!=` is its negation (compiler.go:177), hence true for nil.
  * `<  <=  >  >=` are compareValues (compiler.go:268-322): a number on both sides (:288-303) or a string on both
    sides, compared bytewise on UTF-8 (:304-319); anything else -- nil, a bool, a number against a string -- is an
    error (:321, :290-293, :306-309).
  * `IN` is DeepEqual against any list item (compiler.go:377-391), `NOT IN` its negation (:208-213); neither errors.
  * STARTS_WITH, ENDS_WITH and CONTAINS need two strings, otherwise an error (compiler.go:393-418).
  * MATCHES needs two strings as well, otherwise an error, and is regexp.MatchString(pattern, value)
    (compiler.go:220, :420-431): an unanchored search.  Deviation: the pattern is compiled here, when the expression
    is built (regex_dfa.py), and one outside that module's subset of RE2 -- flags such as (?i), \\b, \\p{..}, \\x,
    named groups -- or one RE2 itself rejects raises ValueError there.  The reference would evaluate the former and
    fail every row on the latter; for those, SearchArgs.Filter remains the route.
  * An error ANYWHERE makes the row fail: both operands of AND and of OR are evaluated before the operator is applied
    (compiler.go:32-45), so `a OR b` fails when b errors even if a is true, and NOT of an error is an error
    (CreateFilterFunction turns the error into false, compiler.go:485-488).

Hence on the device: result = V(expr) & valid_docs & the conjunction of present(field) over every leaf that can error,
where V is plain mask algebra over the leaves (collection.py).

Out of scope: LENGTH, ANY / ALL, nested paths, EXISTS / DOES NOT EXIST.  The reference's lexer has no
negative number literal (query/lexer.go:156): text() writes one as `-5`, which only this module's parse() reads back.
"""
import json
import math

from . import regex_dfa

__all__ = ["Field", "Expr", "parse", "parse_metadata"]

_ORDERED = ("<", "<=", ">", ">=")
_STRING_OPS = ("STARTS_WITH", "ENDS_WITH", "CONTAINS")


class _Error(Exception):
    """An evaluation error of the reference: the row fails whatever the rest of the expression says."""


def _reject_constant(name):
    raise ValueError("not JSON: %s" % name)   # Go's encoding/json knows no NaN / Infinity literals


def _json_float(text):
    f = float(text)
    if not math.isfinite(f):
        raise ValueError("number out of range")   # json.Unmarshal: strconv.ParseFloat's range error fails the document
    return f


def _json_int(text):
    i = int(text)
    try:
        float(i)
    except OverflowError:
        raise ValueError("number out of range")
    return i


def parse_metadata(metadata):
    """The metadata as the reference's filters see it: a dict, or None when json.Unmarshal would fail or the value is
    not a JSON object."""
    try:
        if isinstance(metadata, (bytes, bytearray, memoryview)):
            metadata = bytes(metadata).decode("utf-8", "replace")   # (Go replaces invalid UTF-8 with U+FFFD)
        data = json.loads(metadata, parse_constant=_reject_constant, parse_float=_json_float, parse_int=_json_int)
    except (ValueError, RecursionError):
        return None
    return data if isinstance(data, dict) else None


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _number(v):
    """A JSON number as Go's float64 (parse_metadata has rejected the documents whose numbers are out of range)."""
    return float(v)


def _constant(c):
    if isinstance(c, str):
        return c
    if _is_number(c) or (hasattr(c, "__float__") and not isinstance(c, bool)):
        f = float(c)
        if not math.isfinite(f):
            raise ValueError("the filter language has no literal for %r" % (c,))
        return f
    raise TypeError("a filter constant is a number or a string, not %r" % (c,))


def _deep_equal(v, c):
    if isinstance(c, float):
        return _is_number(v) and float(v) == c
    return isinstance(v, str) and v == c


def _bytes(s):
    return s.encode("utf-8", "surrogatepass")


def _number_text(f):
    if f == int(f) and abs(f) < 1e15 and not (f == 0 and math.copysign(1.0, f) < 0):
        return str(int(f))
    return repr(f)


def _string_text(s):
    out = s.replace("\\", "\\\\").replace('"', '\\"').replace("\n", "\\n").replace("\t", "\\t").replace("\r", "\\r")
    return '"%s"' % out


def _constant_text(c):
    return _number_text(c) if isinstance(c, float) else _string_text(c)


class Expr:
    """A filter expression; combine with & | ~."""

    def __and__(self, other):
        return And(self, _expr(other))

    def __or__(self, other):
        return Or(self, _expr(other))

    def __invert__(self):
        return Not(self)

    def __bool__(self):
        raise TypeError("combine filter expressions with & | ~ (and parenthesise comparisons), not and / or / not")

    def text(self):
        """The filter in the reference's filter language."""
        raise NotImplementedError

    def fields(self):
        """The metadata fields the expression reads."""
        raise NotImplementedError

    def _eval(self, data):
        raise NotImplementedError

    def evaluate(self, metadata):
        """The reference's verdict on one document's metadata bytes."""
        data = parse_metadata(metadata)
        if data is None:
            return False
        try:
            return self._eval(data)
        except _Error:
            return False

    def __repr__(self):
        return "<where %s>" % self.text()


def _expr(e):
    if not isinstance(e, Expr):
        raise TypeError("not a filter expression: %r" % (e,))
    return e


def _value(data, name):
    """The field as Go sees it after json.Unmarshal: None, bool, float, str, list or dict."""
    v = data.get(name)
    return _number(v) if _is_number(v) else v


class Cmp(Expr):
    """field op constant, op one of == != < <= > >=."""

    def __init__(self, field, op, constant):
        if op not in ("==", "!=") + _ORDERED:
            raise ValueError("unknown comparison %r" % (op,))
        self.field, self.op, self.constant = field, op, _constant(constant)

    def text(self):
        return "%s %s %s" % (self.field, self.op, _constant_text(self.constant))

    def fields(self):
        return {self.field}

    def test(self, v):
        """The comparison on one value of the field (None, bool, float, str, list, dict); raises on an error."""
        c = self.constant
        if self.op == "==":
            return _deep_equal(v, c)
        if self.op == "!=":
            return not _deep_equal(v, c)
        if _is_number(v) and isinstance(c, float):
            a, b = float(v), c
        elif isinstance(v, str) and isinstance(c, str):
            a, b = _bytes(v), _bytes(c)
        else:
            raise _Error("unsupported comparison")
        return {"<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[self.op]

    def _eval(self, data):
        return self.test(_value(data, self.field))


class In(Expr):
    """field IN [constants] / field NOT IN [constants]."""

    def __init__(self, field, constants, negate=False):
        self.field, self.constants, self.negate = field, [_constant(c) for c in constants], bool(negate)

    def text(self):
        return "%s %s [%s]" % (self.field, "NOT IN" if self.negate else "IN",
                               ", ".join(_constant_text(c) for c in self.constants))

    def fields(self):
        return {self.field}

    def test(self, v):
        return any(_deep_equal(v, c) for c in self.constants) != self.negate

    def _eval(self, data):
        return self.test(_value(data, self.field))


class StrOp(Expr):
    """field STARTS_WITH / ENDS_WITH / CONTAINS "constant"."""

    def __init__(self, field, op, constant):
        if op not in _STRING_OPS:
            raise ValueError("unknown string operator %r" % (op,))
        if not isinstance(constant, str):
            raise TypeError("%s takes a string constant" % op)
        self.field, self.op, self.constant = field, op, constant

    def text(self):
        return "%s %s %s" % (self.field, self.op, _string_text(self.constant))

    def fields(self):
        return {self.field}

    def test(self, v):
        if not isinstance(v, str):
            raise _Error("%s requires string operands" % self.op)
        a, b = _bytes(v), _bytes(self.constant)
        if self.op == "STARTS_WITH":
            return a.startswith(b)
        if self.op == "ENDS_WITH":
            return a.endswith(b)
        return b in a

    def _eval(self, data):
        return self.test(_value(data, self.field))


class Matches(Expr):
    """field MATCHES "pattern": Go's regexp.MatchString on a string value (the subset of regex_dfa)."""

    def __init__(self, field, pattern):
        if not isinstance(pattern, str):
            raise TypeError("MATCHES takes a string constant")
        self.field, self.pattern = field, pattern
        self.matcher = regex_dfa.matcher(pattern)   # ValueError: outside the subset, or not a regular expression

    def text(self):
        return "%s MATCHES %s" % (self.field, _string_text(self.pattern))

    def fields(self):
        return {self.field}

    def test(self, v):
        if not isinstance(v, str):
            raise _Error("MATCHES requires string operands")
        return self.matcher.match(_bytes(v))

    def _eval(self, data):
        return self.test(_value(data, self.field))


class And(Expr):
    def __init__(self, a, b):
        self.a, self.b = a, b

    def text(self):
        return "(%s AND %s)" % (self.a.text(), self.b.text())

    def fields(self):
        return self.a.fields() | self.b.fields()

    def _eval(self, data):
        a, b = self.a._eval(data), self.b._eval(data)   # both, before the operator: an error on either side wins
        return a and b


class Or(Expr):
    def __init__(self, a, b):
        self.a, self.b = a, b

    def text(self):
        return "(%s OR %s)" % (self.a.text(), self.b.text())

    def fields(self):
        return self.a.fields() | self.b.fields()

    def _eval(self, data):
        a, b = self.a._eval(data), self.b._eval(data)
        return a or b


class Not(Expr):
    def __init__(self, a):
        self.a = a

    def text(self):
        return "NOT (%s)" % self.a.text()

    def fields(self):
        return self.a.fields()

    def _eval(self, data):
        return not self.a._eval(data)


class Field:
    """A top-level metadata field: compare it with a number or a string to get an expression."""
    __hash__ = None

    def __init__(self, name):
        if not isinstance(name, str) or not name or not (name[0].isalpha() or name[0] == "_") or \
                not all(ch.isascii() and (ch.isalnum() or ch == "_") for ch in name):
            raise ValueError("a field name is an identifier of the filter language (letters, digits, _): %r" % (name,))
        self.name = name

    def __lt__(self, c):
        return Cmp(self.name, "<", c)

    def __le__(self, c):
        return Cmp(self.name, "<=", c)

    def __gt__(self, c):
        return Cmp(self.name, ">", c)

    def __ge__(self, c):
        return Cmp(self.name, ">=", c)

    def __eq__(self, c):
        return Cmp(self.name, "==", c)

    def __ne__(self, c):
        return Cmp(self.name, "!=", c)

    def isin(self, constants):
        return In(self.name, constants)

    def notin(self, constants):
        return In(self.name, constants, negate=True)

    def startswith(self, s):
        return StrOp(self.name, "STARTS_WITH", s)

    def endswith(self, s):
        return StrOp(self.name, "ENDS_WITH", s)

    def contains(self, s):
        return StrOp(self.name, "CONTAINS", s)

    def matches(self, pattern):
        return Matches(self.name, pattern)


# ---- text -> tree, for the subset text() writes (query/lexer.go, query/parser.go: OR < AND < comparison < NOT) --------

_KEYWORDS = ("AND", "OR", "NOT", "IN", "MATCHES") + _STRING_OPS


def _tokens(text):
    i, n = 0, len(text)
    while i < n:
        ch = text[i]
        if ch in " \t\r\n":
            i += 1
        elif ch in "()[],":
            yield (ch, ch)
            i += 1
        elif text.startswith(("==", "!=", "<=", ">="), i):
            yield ("op", text[i:i + 2])
            i += 2
        elif ch in "<>":
            yield ("op", ch)
            i += 1
        elif ch in "\"'":
            quote, out = ch, []
            i += 1
            while i < n and text[i] != quote:
                if text[i] == "\\" and i + 1 < n:
                    i += 1
                    out.append({"n": "\n", "t": "\t", "r": "\r", "\\": "\\", '"': '"'}.get(text[i], "\\" + text[i]))
                else:
                    out.append(text[i])
                i += 1
            if i >= n:
                raise ValueError("unterminated string in filter")
            i += 1
            yield ("str", "".join(out))
        elif ch.isdigit() or (ch == "-" and i + 1 < n and text[i + 1].isdigit()):
            j = i + 1
            while j < n and (text[j].isdigit() or text[j] in ".eE" or (text[j] in "+-" and text[j - 1] in "eE")):
                j += 1
            yield ("num", float(text[i:j]))
            i = j
        elif ch.isalpha() or ch == "_":
            j = i
            while j < n and (text[j].isalnum() or text[j] == "_"):
                j += 1
            word = text[i:j]
            yield ("kw", word) if word in _KEYWORDS else ("id", word)
            i = j
        else:
            raise ValueError("unexpected %r in filter" % ch)
    yield ("eof", None)


class _Parser:
    def __init__(self, text):
        self.toks = list(_tokens(text))
        self.i = 0

    def peek(self):
        return self.toks[self.i]

    def take(self, kind=None, value=None):
        t = self.toks[self.i]
        if (kind is not None and t[0] != kind) or (value is not None and t[1] != value):
            raise ValueError("filter: expected %s, got %r" % (value or kind, t[1]))
        self.i += 1
        return t

    def parse_or(self):
        e = self.parse_and()
        while self.peek() == ("kw", "OR"):
            self.take()
            e = Or(e, self.parse_and())
        return e

    def parse_and(self):
        e = self.parse_not()
        while self.peek() == ("kw", "AND"):
            self.take()
            e = And(e, self.parse_not())
        return e

    def parse_not(self):
        if self.peek() == ("kw", "NOT"):
            self.take()
            return Not(self.parse_primary())
        return self.parse_primary()

    def constant(self):
        t = self.take()
        if t[0] not in ("num", "str"):
            raise ValueError("filter: expected a number or a string, got %r" % (t[1],))
        return t[1]

    def parse_primary(self):
        if self.peek()[0] == "(":
            self.take()
            e = self.parse_or()
            self.take(")")
            return e
        name = self.take("id")[1]
        kind, what = self.take()
        if kind == "op":
            return Cmp(name, what, self.constant())
        if kind == "kw" and what in _STRING_OPS:
            return StrOp(name, what, self.take("str")[1])
        if (kind, what) == ("kw", "MATCHES"):
            return Matches(name, self.take("str")[1])
        negate = (kind, what) == ("kw", "NOT")
        if negate:
            kind, what = self.take()
        if (kind, what) != ("kw", "IN"):
            raise ValueError("filter: expected an operator after %s, got %r" % (name, what))
        self.take("[")
        items = []
        if self.peek()[0] != "]":
            items.append(self.constant())
            while self.peek()[0] == ",":
                self.take()
                items.append(self.constant())
        self.take("]")
        return In(name, items, negate)


def parse(text):
    """The tree of a filter text, for the subset of the language this module writes."""
    p = _Parser(text)
    e = p.parse_or()
    p.take("eof")
    return e
