"""The pinned runs of scripts/fuzz_state.py: what tests/test_gpu_fuzz_state.py runs on the card and what
tests/test_fuzz_state_cpu.py holds the generator to.  Test support: nothing on the search path imports it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "fuzz_state.py")
if os.path.dirname(SCRIPT) not in sys.path:
    sys.path.insert(0, os.path.dirname(SCRIPT))
import fuzz_state  # noqa: E402,F401 -- the script as a module: its checkers and its operation kinds (numpy only)

PINS = [("plain", 21), ("plain", 22), ("sketched", 31), ("sketched", 32)]

# Cases per run: a count, not a time, so a seed means the same cases on every run and every card.  The largest multiple of
# 10 at which each of the four runs takes about 10 s of wall time on an MI355X, the oracle's CPU time and the start of the
# interpreter included (the budget follows the 12 s that test_fuzz_short's count was sized from).
# Measured on an MI355X, the script alone: 110 cases take 5.3 s (plain 21), 6.6 s (plain 22), 8.6 s (sketched 31) and 10.4 s
# (sketched 32); 100 cases took 5.4, 6.1, 8.2 and 9.5 s.  120 was not measured: at sketched 32's 0.09 s per case it would
# take about 11.3 s.  (test_gpu_fuzz_state.py also runs the plan of each seed without the card, 2 to 4 s more.)
CASES = 110


def command(profile, seed, *more):
    return [sys.executable, SCRIPT, str(seed), "--cases", str(CASES), "--profile", profile, *more]
