"""The option table (syzgydb_amd/csrc/options.h + options.cpp) without a GPU.

A stand-alone program (tests/cpp/test_options.cpp, plain g++, its own main) is built from options.cpp and scan_plan.cpp
alone and runs under the address and undefined-behaviour sanitizers: names, defaults, flags, edge values, what they store
and the refusals' texts, against a list written out by hand from the setter's if-chains before the table.  The same
list, in Python (option_cases.py), is what szg_debug_option_check is held to through the loaded library -- which may be
an older build's (SZG_LIB_PATH): the list states what the setter always did."""
import os
import shutil
import subprocess

import pytest

import option_cases as oc
from syzgydb_amd import SzgError, _lib
from syzgydb_amd.index import option_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "syzgy_scan.h")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_options.cpp"
    exe = str(tmp_path_factory.mktemp("options") / "test_options")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_options.cpp"),
                    os.path.join(ROOT, "syzgydb_amd", "csrc", "options.cpp"),
                    os.path.join(ROOT, "syzgydb_amd", "csrc", "scan_plan.cpp")], check=True)
    return exe


def test_standalone_options_program_is_clean_under_sanitizers(program):
    done = subprocess.run([program, HEADER], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "options ok" in done.stdout


def test_the_two_hand_written_lists_are_one(program):
    done = subprocess.run([program, HEADER, "--list"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.splitlines() == oc.listing()


@pytest.mark.parametrize("name", oc.ONE_SWEEP)
def test_option_check_answers_as_the_setter_did(name):
    case = oc.CASES[name]
    for value in range(-2, 1031):
        if value in case["ok"]:
            option_check(name, value)
            continue
        with pytest.raises(SzgError) as e:
            option_check(name, value)
        assert e.value.code == _lib.SZG_E_INVALID and case["text"] in str(e.value), (name, value, str(e.value))
    for value, _ in case["accepted"]:
        option_check(name, value)
    for value in case["refused"]:
        with pytest.raises(SzgError, match=case["text"]):
            option_check(name, value)


@pytest.mark.parametrize("name", ["mq_min", "sketch", "contexts", "nonsense", ""])
def test_option_check_knows_the_one_sweep_options_only(name):
    for value in (0, 1, 2):
        with pytest.raises(SzgError, match="not an option of the one-sweep kernel") as e:
            option_check(name, value)
        assert e.value.code == _lib.SZG_E_INVALID


def test_option_check_of_a_null_name():
    L = _lib.load()
    assert L.szg_debug_option_check(None, 0) == _lib.SZG_E_INVALID
    assert b"null argument" in L.szg_last_error()
