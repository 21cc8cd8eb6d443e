"""Who owns device memory, the parts that need no GPU: the C symbols of the two test hooks, their host-only behaviour,
and the stand-alone program that runs the owning buffers (syzgydb_amd/csrc/dev_mem.h) over a malloc backend under the
sanitizers.  test_gpu_owned_memory.py has the device side."""
import ctypes
import os
import re
import shutil
import subprocess

from syzgydb_amd import _lib
from syzgydb_amd.index import device_memory, refuse_device_alloc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEMORY_SYMBOLS = ["szg_debug_device_memory", "szg_debug_refuse_device_alloc"]


def test_symbols():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "syzgy_scan.h")).read()
    for name in MEMORY_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared in the header" % name
    assert L.szg_abi_version() == 4


def test_hooks_on_the_host():
    L = _lib.load()
    before = device_memory()   # (nothing below allocates: arming and disarming the countdown is host work)
    assert L.szg_debug_device_memory(None, None) == _lib.SZG_OK
    assert L.szg_debug_refuse_device_alloc(-1) == _lib.SZG_E_INVALID
    with refuse_device_alloc(3):
        pass   # armed, and disarmed on exit
    try:
        with refuse_device_alloc(1):
            raise KeyError("x")
    except KeyError:
        pass   # ... on an exception as well
    assert device_memory() == before


def test_no_allocation_by_hand_outside_the_owner():
    """One search confirms it: no hipMalloc( / hipFree( in the library's sources outside dev_mem.h and the exchange's
    staging (scan_comm.cpp)."""
    src = os.path.join(ROOT, "syzgydb_amd", "csrc")
    for name in sorted(os.listdir(src)):
        if name in ("dev_mem.h", "scan_comm.cpp") or not name.endswith((".cpp", ".h", ".hip")):
            continue
        text = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', open(os.path.join(src, name)).read())   # (error texts name the call)
        assert "hipMalloc(" not in text and "hipFree(" not in text, name


def test_standalone_dev_mem_program_is_clean_under_sanitizers(tmp_path):
    """dev_mem.h in a stand-alone program with its own main, plain g++, over a malloc backend that records the current
    device and aborts when a block is freed under another: ensure (no-op, grow, free first), alloc_exact sizes, moves
    between devices, the growth shape (one free of the old block, after the copy), a vector of parts reallocating, the
    countdown, the counters back at 0; a leak is a non-zero exit."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_dev_mem.cpp"
    exe = str(tmp_path / "test_dev_mem")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_dev_mem.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "dev mem ok" in done.stdout


class _FakeLib:
    """Records the destroy calls the wrappers make (no device, no library)."""

    def __init__(self):
        self.calls = []

    def szg_mask_destroy(self, h):
        self.calls.append(("mask", h.value))

    def szg_column_destroy(self, h):
        self.calls.append(("column", h.value))

    def szg_index_destroy(self, h):
        self.calls.append(("index", h.value))


def test_a_garbage_cycle_destroys_masks_and_columns_before_their_index():
    """The cycle collector clears weak references before it runs __del__, in no useful order: an index that is garbage
    together with its masks and columns must still destroy them first (szg_mask_destroy updates counters inside its
    index: after szg_index_destroy that is a write into freed memory), and each handle exactly once."""
    import gc
    from syzgydb_amd.index import ScanColumn, ScanIndex, ScanMask
    L = _FakeLib()
    ix = object.__new__(ScanIndex)
    ix._L, ix._h, ix._masks, ix._columns, ix._comm = L, ctypes.c_void_p(1), {}, {}, None
    m = ScanMask(ix, ctypes.c_void_p(2), 1)
    c = ScanColumn(ix, ctypes.c_void_p(3), _lib.SZG_COL_F64)
    closed = ScanMask(ix, ctypes.c_void_p(4), 1)
    closed.close()
    cycle = [ix, m, c, closed]
    cycle.append(cycle)
    del ix, m, c, closed, cycle
    gc.collect()
    assert sorted(L.calls) == [("column", 3), ("index", 1), ("mask", 2), ("mask", 4)]
    assert L.calls[0] == ("mask", 4) and L.calls[-1] == ("index", 1)
