"""The one-sweep scan's plan without HIP and without a GPU (syzgydb_amd/csrc/scan_plan.h + scan_plan.cpp): which kernel a
launch takes, its LDS bytes and the merges' shapes.  A stand-alone program (tests/cpp/test_scan_plan.cpp, plain g++, its
own main) is built from those two files alone and runs under the address and undefined-behaviour sanitizers; what it
expects for the sketch's launches, the shape kernels of each width and the merges' edges is written out by hand."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_standalone_scan_plan_program_is_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_scan_plan.cpp"
    exe = str(tmp_path / "test_scan_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_scan_plan.cpp"),
                    os.path.join(ROOT, "syzgydb_amd", "csrc", "scan_plan.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "scan plan ok" in done.stdout
