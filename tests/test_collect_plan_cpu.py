"""The buffer arithmetic of a radius batch without a GPU (syzgydb_amd/csrc/collect_plan.h): the sizes and offsets that
index a batch's collect buffers, counters and pinned hits.  A stand-alone program (tests/cpp/test_collect_plan.cpp, plain
g++, its own main) allocates buffers of exactly the sizes the header computes, writes and reads every list at the
offsets it gives, and runs under the address and undefined-behaviour sanitizers; the cap sequence it expects is written
out by hand."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_standalone_collect_plan_program_is_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_collect_plan.cpp"
    exe = str(tmp_path / "test_collect_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_collect_plan.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "collect plan ok" in done.stdout
