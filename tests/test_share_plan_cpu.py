"""The matrix sweep's shared form as the plan header states it, without HIP and without a GPU (syzgydb_amd/csrc/scan_plan.h +
scan_plan.cpp): share_map is a bijection from the blocks of an even grid onto (row slice, column group), partners are b
and b + 8 where 16 divides the grid, the lists of 33 to 64 queries tile a buffer of nq * S * m entries exactly, every
tile is visited once per group, and scan_variant names the form for exactly the launches it serves.  A stand-alone
program (tests/cpp/test_share_plan.cpp, plain g++, its own main) runs under the address and undefined-behaviour
sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_standalone_share_plan_program_is_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_share_plan.cpp"
    exe = str(tmp_path / "test_share_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_share_plan.cpp"),
                    os.path.join(ROOT, "syzgydb_amd", "csrc", "scan_plan.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "share plan ok" in done.stdout
