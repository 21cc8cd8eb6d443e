"""The plan of a call through the sketch as its header states it, without HIP and without a GPU
(syzgydb_amd/csrc/sketch_plan.h over scan_plan.h + scan_plan.cpp): the batches of the automatic rule and of the forced
plans, the call rule's thresholds at 72 and 136 queries, the early tail of a short call, and for every call of 1 to 200
queries under every wide / share that its launches partition the call, keep within 16, 32 or 64 queries as their form
allows and make one pass per group.  The launch path and the plan hooks compute from the same functions.  A stand-alone
program (tests/cpp/test_sketch_plan.cpp, plain g++, its own main) runs under the address and undefined-behaviour
sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_standalone_sketch_plan_program_is_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_sketch_plan.cpp"
    exe = str(tmp_path / "test_sketch_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_sketch_plan.cpp"),
                    os.path.join(ROOT, "syzgydb_amd", "csrc", "scan_plan.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "sketch plan ok" in done.stdout
