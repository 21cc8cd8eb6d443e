"""Resident metadata columns, the parts that need no GPU: the C symbols and their argument checks, and where.evaluate --
the host restatement of the reference's filter rules that the device path is tested against (test_gpu_columns.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from syzgydb_amd import _lib
from syzgydb_amd.where import Field, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COLUMN_SYMBOLS = ["szg_column_create", "szg_column_append", "szg_column_set", "szg_column_rows", "szg_column_read",
                  "szg_column_destroy", "szg_mask_where_f64", "szg_mask_where_in_f64", "szg_mask_where_u32",
                  "szg_mask_where_present"]


def test_symbols_resolve_and_abi_stays_4():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "syzgy_scan.h")).read()
    for name in COLUMN_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared in the header" % name
    assert L.szg_abi_version() == 4
    assert (_lib.SZG_COL_F64, _lib.SZG_COL_U32) == (0, 1)
    assert [_lib.SZG_CMP_EQ, _lib.SZG_CMP_NE, _lib.SZG_CMP_LT, _lib.SZG_CMP_LE, _lib.SZG_CMP_GT, _lib.SZG_CMP_GE] == list(range(6))
    for name, value in (("SZG_COL_F64", 0), ("SZG_COL_U32", 1), ("SZG_CMP_EQ", 0), ("SZG_CMP_NE", 1), ("SZG_CMP_LT", 2),
                        ("SZG_CMP_LE", 3), ("SZG_CMP_GT", 4), ("SZG_CMP_GE", 5)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name


def test_null_and_invalid_arguments_are_rejected_on_the_host():
    """Every check precedes device work: these calls run on a machine without a GPU."""
    L = _lib.load()
    out = ctypes.c_void_p(0x1234)   # must stay untouched by a failing call
    one = (ctypes.c_double * 1)(1.0)
    bits = (ctypes.c_uint64 * 1)(1)
    assert L.szg_column_create(None, _lib.SZG_COL_F64, one, None, 1, ctypes.byref(out)) == _lib.SZG_E_INVALID
    assert b"null" in L.szg_last_error()
    assert L.szg_column_append(None, one, None, 1) == _lib.SZG_E_INVALID
    assert L.szg_column_set(None, 0, one) == _lib.SZG_E_INVALID
    assert L.szg_column_read(None, 0, 0, None, None) == _lib.SZG_E_INVALID
    assert L.szg_column_rows(None) == 0
    L.szg_column_destroy(None)
    assert L.szg_mask_where_f64(None, _lib.SZG_CMP_LT, 1.0, None, ctypes.byref(out)) == _lib.SZG_E_INVALID
    for op in (-1, 6, 100):
        assert L.szg_mask_where_f64(None, op, 1.0, None, ctypes.byref(out)) == _lib.SZG_E_INVALID
        assert b"operator" in L.szg_last_error()
    assert L.szg_mask_where_in_f64(None, one, 1, None, ctypes.byref(out)) == _lib.SZG_E_INVALID
    assert L.szg_mask_where_in_f64(None, None, 1, None, ctypes.byref(out)) == _lib.SZG_E_INVALID
    many = (ctypes.c_double * 1025)()
    assert L.szg_mask_where_in_f64(None, many, 1025, None, ctypes.byref(out)) == _lib.SZG_E_UNSUPPORTED
    assert L.szg_mask_where_u32(None, bits, 1, None, ctypes.byref(out)) == _lib.SZG_E_INVALID
    assert L.szg_mask_where_u32(None, None, 1, None, ctypes.byref(out)) == _lib.SZG_E_INVALID
    assert L.szg_mask_where_present(None, None, ctypes.byref(out)) == _lib.SZG_E_INVALID
    assert out.value == 0x1234


def test_standalone_bit_copy_program_is_clean_under_sanitizers(tmp_path):
    """szg_column_append shifts the caller's present bits into place (column_bits.h): a stand-alone program, plain g++
    with its own main, checks that routine against a bit-by-bit restatement on buffers sized exactly for their bits."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_column_bits.cpp"
    exe = str(tmp_path / "test_column_bits")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_column_bits.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "column bits ok" in done.stdout


price, name, flag = Field("price"), Field("name"), Field("flag")

# (expression, metadata, verdict, the reference line that decides it)
TRUTH = [
    # a number field against a number constant: float64 == and <  (compiler.go:175 DeepEqual, :288-303)
    (price == 5, b'{"price": 5}', True, "compiler.go:175"),
    (price == 5, b'{"price": 5.0}', True, "compiler.go:175 (json numbers are float64)"),
    (price == 5, b'{"price": 6}', False, "compiler.go:175"),
    (price != 5, b'{"price": 6}', True, "compiler.go:177"),
    (price != 5, b'{"price": 5}', False, "compiler.go:177"),
    (price < 5, b'{"price": 4.5}', True, "compiler.go:299-300"),
    (price < 5, b'{"price": 5}', False, "compiler.go:299-300"),
    (price <= 5, b'{"price": 5}', True, "compiler.go:301-302"),
    (price > 5, b'{"price": 5}', False, "compiler.go:295-296"),
    (price >= 5, b'{"price": 5}', True, "compiler.go:297-298"),
    (price > 5, b'{"price": 1e3}', True, "compiler.go:295-296"),
    # -0.0 == 0 by float64 ==
    (price == 0, b'{"price": -0.0}', True, "compiler.go:175 (DeepEqual on float64 is ==)"),
    (price < 0, b'{"price": -0.0}', False, "compiler.go:299-300"),
    # absent field = nil (compiler.go:438 map lookup)
    (price == 5, b'{"other": 1}', False, "compiler.go:438, :175"),
    (price != 5, b'{"other": 1}', True, "compiler.go:438, :177"),
    (price < 5, b'{"other": 1}', False, "compiler.go:321 (nil is no comparable kind: error)"),
    (price >= 5, b'{}', False, "compiler.go:321"),
    # null = nil
    (price == 5, b'{"price": null}', False, "compiler.go:175"),
    (price != 5, b'{"price": null}', True, "compiler.go:177"),
    (price > 5, b'{"price": null}', False, "compiler.go:321"),
    # number field vs string constant, and string field vs number constant
    (price == "5", b'{"price": 5}', False, "compiler.go:175 (float64 vs string)"),
    (price != "5", b'{"price": 5}', True, "compiler.go:177"),
    (price < "5", b'{"price": 4}', False, "compiler.go:290-293 (toFloat64 of a string: error)"),
    (name == 5, b'{"name": "5"}', False, "compiler.go:175"),
    (name != 5, b'{"name": "5"}', True, "compiler.go:177"),
    (name < 5, b'{"name": "4"}', False, "compiler.go:306-309 (string vs non-string: error)"),
    # a bool value
    (flag == 1, b'{"flag": true}', False, "compiler.go:175 (bool vs float64)"),
    (flag != 1, b'{"flag": true}', True, "compiler.go:177"),
    (flag < 1, b'{"flag": false}', False, "compiler.go:321 (bool is no comparable kind: error)"),
    (flag.isin([1, "true"]), b'{"flag": true}', False, "compiler.go:385"),
    # arrays and objects as values
    (price == 5, b'{"price": [5]}', False, "compiler.go:175"),
    (price < 5, b'{"price": {"a": 1}}', False, "compiler.go:321"),
    # metadata that is not an object, or not JSON at all
    (price != 5, b'[1, 2]', False, "compiler.go:445 (getField on a non-map: error)"),
    (price != 5, b'5', False, "compiler.go:445"),
    (price != 5, b'"price"', False, "compiler.go:445"),
    (price != 5, b'null', False, "compiler.go:445"),
    (price != 5, b'', False, "compiler.go:480-483 (json.Unmarshal fails)"),
    (price != 5, b'{"price": 5', False, "compiler.go:480-483"),
    (price != 5, b'doc7', False, "compiler.go:480-483"),
    (price != 5, b'{"price": NaN}', False, "compiler.go:480-483 (no NaN literal in JSON)"),
    # strings: == by bytes, ordering bytewise on UTF-8
    (name == "abc", b'{"name": "abc"}', True, "compiler.go:175"),
    (name == "abc", b'{"name": "abd"}', False, "compiler.go:175"),
    (name != "abc", b'{"name": "abd"}', True, "compiler.go:177"),
    (name < "b", b'{"name": "abc"}', True, "compiler.go:315-316"),
    (name >= "b", b'{"name": "abc"}', False, "compiler.go:313-314"),
    (name < "abc", b'{"name": "ab"}', True, "compiler.go:315-316 (a prefix sorts first)"),
    (name > "z", '{"name": "é"}'.encode(), True, "compiler.go:311-312 (0xC3 0xA9 > 0x7A bytewise)"),
    (name < "é", b'{"name": "zz"}', True, "compiler.go:315-316"),
    (name < "\U0001F600", '{"name": "�"}'.encode(), True, "compiler.go:315-316 (0xEF.. < 0xF0.. bytewise)"),
    (name == "é", b'{"name": "\\u00e9"}', True, "compiler.go:175 (escapes decode to the same bytes)"),
    # IN / NOT IN: DeepEqual against any item, never an error
    (price.isin([1, 5, 9]), b'{"price": 5}', True, "compiler.go:385"),
    (price.isin([1, 9]), b'{"price": 5}', False, "compiler.go:390"),
    (price.isin([]), b'{"price": 5}', False, "compiler.go:390"),
    (price.isin([1, "5"]), b'{"price": "5"}', True, "compiler.go:385"),
    (price.isin([1, 5]), b'{}', False, "compiler.go:390 (nil equals no item)"),
    (price.notin([1, 5]), b'{}', True, "compiler.go:208-213 (NOT IN on an absent field)"),
    (price.notin([1, 5]), b'{"price": 5}', False, "compiler.go:208-213"),
    (price.notin([1, 5]), b'[5]', False, "compiler.go:445"),
    (name.isin(["a", "b"]), b'{"name": "b"}', True, "compiler.go:385"),
    # string operators need two strings
    (name.startswith("ab"), b'{"name": "abc"}', True, "compiler.go:408"),
    (name.startswith("bc"), b'{"name": "abc"}', False, "compiler.go:408"),
    (name.endswith("bc"), b'{"name": "abc"}', True, "compiler.go:417"),
    (name.contains("b"), b'{"name": "abc"}', True, "compiler.go:399"),
    (name.contains(""), b'{"name": ""}', True, "compiler.go:399"),
    (name.contains("x"), b'{"name": "abc"}', False, "compiler.go:399"),
    (name.startswith("1"), b'{"name": 12}', False, "compiler.go:405-407 (error)"),
    (name.contains("a"), b'{}', False, "compiler.go:396-398 (nil: error)"),
    # an error anywhere fails the row: both operands are evaluated first (compiler.go:32-45)
    ((price == 5) | (name < "b"), b'{"price": 5, "name": "a"}', True, "compiler.go:187-199"),
    ((price == 5) | (name < "b"), b'{"price": 5}', False, "compiler.go:37-40 (a OR b, b errors, a true)"),
    ((name < "b") | (price == 5), b'{"price": 5}', False, "compiler.go:33-36"),
    ((price == 5) & (name < "b"), b'{"price": 4}', False, "compiler.go:37-40"),
    ((price == 4) & (name < "b"), b'{"price": 4, "name": "a"}', True, "compiler.go:180-186"),
    (~(price < 5), b'{"price": 7}', True, "compiler.go:200-205"),
    (~(price < 5), b'{"price": 3}', False, "compiler.go:200-205"),
    (~(price < 5), b'{}', False, "compiler.go:37-40 (NOT of an error is an error)"),
    (~(price < 5), b'{"price": "3"}', False, "compiler.go:37-40"),
    (~(price == 5), b'{}', True, "compiler.go:175, :205 (== never errors)"),
    (~(~(name.startswith("a"))), b'{"name": 1}', False, "compiler.go:37-40"),
    ((price != 5) | ~(name.contains("a")), b'{"name": 3}', False, "compiler.go:37-40"),
]


@pytest.mark.parametrize("case", range(len(TRUTH)))
def test_evaluate_truth_table(case):
    """where.evaluate against verdicts derived by hand from the reference's compiler; TRUTH names, per case, the line
    that decides it.  Covered: absent field, null, number-vs-string mismatch in both directions, a bool value,
    non-object and empty metadata, `a OR b` with b erroring, ~ of an erroring leaf, -0.0 == 0, NOT IN on an absent
    field, a non-ASCII string ordering."""
    expr, meta, want, cite = TRUTH[case]
    assert expr.evaluate(meta) is want, (expr.text(), meta, cite)


def test_text_round_trips_for_each_operator():
    exprs = [price == 5, price != 5.5, price < 1e20, price <= 0.001, price > 3, price >= 37.5,
             name == "a b", name != 'q"uote\\', name < "é", name >= "tab\there\n",
             price.isin([1, 2.5, 3]), price.notin([7]), name.isin(["x", "y"]), name.isin([]), price.isin([1, "one"]),
             name.startswith("pre"), name.endswith("post"), name.contains("mid"),
             (price < 5) & (name == "a"), (price < 5) | (name == "a"), ~(price < 5),
             ~((price < 5) & ((name == "a") | ~name.contains("z"))) | price.notin([1, 2])]
    seen = set()
    for e in exprs:
        text = e.text()
        back = parse(text)
        assert back.text() == text
        assert back.fields() == e.fields()
        for _, meta, _, _ in TRUTH:
            assert back.evaluate(meta) == e.evaluate(meta), (text, meta)
        seen.add(text)
    assert len(seen) == len(exprs)
    assert (price < 37.5).text() == "price < 37.5"
    assert (name == "x").text() == 'name == "x"'
    assert price.notin([1, 2]).text() == "price NOT IN [1, 2]"
    assert name.startswith("a").text() == 'name STARTS_WITH "a"'
    assert ((price < 5) & ~(name == "a")).text() == '(price < 5 AND NOT (name == "a"))'
    assert ((price < 5) | (name == "a")).fields() == {"price", "name"}


def test_expression_construction_errors():
    with pytest.raises(TypeError):
        price < None
    with pytest.raises(TypeError):
        price == True   # noqa: E712
    with pytest.raises(ValueError):
        price < float("nan")
    with pytest.raises(TypeError):
        name.startswith(3)
    with pytest.raises(ValueError):
        Field("a.b")
    with pytest.raises(TypeError):
        (price < 5) & True
    with pytest.raises(TypeError):
        bool(price < 5)


def test_search_args_where_is_exclusive_with_filter():
    from syzgydb_amd import Collection, SearchArgs
    args = SearchArgs(Vector=[0.0], K=1, Filter=lambda id_, meta: True, Where=price < 5)
    with pytest.raises(ValueError):
        Collection._search_filter(None, args)
    assert SearchArgs().Where is None
