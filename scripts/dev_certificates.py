"""The certificate margins: how much of each key bound the kernels use.

Runs tests/test_gpu_certificates.py, tests/test_gpu_sketch_state.py and tests/test_gpu_coincident.py (every claim is
asserted there: a failure fails this script too), then writes the largest |key - real| / eps the run saw per pass kind, arithmetic, row width and
metric -- for the bfloat16 sweeps also the largest |key - emulated key| / (the float32-accumulation part of the bound),
for the sketch sweep's own keys the K_s lines, and per metric and dimension how close the farthest row comes to the
slack the search allows between a row and its sketch (B3) -- to profiles/certificate_margins.txt, with the commit it
measured.  The margins of tests/test_gpu_coincident.py -- queries on stored rows and within a few float32 spacings of
them -- are a section of their own, "keys at and near zero": there the requirement is max ratio <= 1 on every line, and
every family that file forces has to have left one.  A ratio that creeps towards 1 after a kernel change
is margin the change has eaten.

    python scripts/dev_certificates.py [--out profiles/certificate_margins.txt] [--commit NAME] [pytest arguments]

--commit names the commit where the tree is not a git checkout (a copy on a GPU machine).
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]

import pytest  # noqa: E402

import test_gpu_certificates as t  # noqa: E402
import test_gpu_coincident as tz  # noqa: E402
import test_gpu_sketch_state as ts  # noqa: E402

WANT = [("topk", "Single", "one-sweep"), ("radius", "-", "one-sweep"), ("topk", "SharedInt8", "int8"),
        ("radius-shared", "-", "int8"), ("topk", "SharedBf16", "bf16"), ("topk", "Bf16Band", "bf16"),
        ("topk", "Bf16Rescored", "bf16"), ("radius-shared", "-", "bf16"), ("escalation", "-", "one-sweep"),
        ("bf16-operands", "SharedBf16", "topk"), ("bf16-operands", "-", "radius-shared"),
        ("sketch K_s", "Single", "one-sweep")]
# ... and of tests/test_gpu_coincident.py: every family it forces (no escalation is forced there)
WANT_ZERO = [w for w in WANT if w[0] != "escalation"]


merged = t.cc.Margins()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "certificate_margins.txt"))
    ap.add_argument("--commit", default=None)
    args, rest = ap.parse_known_args()
    rc = pytest.main([t.__file__, ts.__file__, tz.__file__, "-m", "gpu", "-q", "-p", "no:cacheprovider"] + rest)
    for m in (t.MARGINS, ts.MARGINS):   # (each file keeps its own)
        for what, ratio in m.worst.items():
            merged.note(what, ratio, m.count[what])
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "describe", "--always", "--dirty"], text=True,
                                             stderr=subprocess.DEVNULL).strip()
        except (OSError, subprocess.CalledProcessError):
            commit = "unknown (no git checkout)"
    kinds = {(p, k, s) for (p, k, s, _, _) in merged.worst}
    missing = [w for w in WANT if w not in kinds]
    missing += [w + ("at zero",) for w in WANT_ZERO if w not in {(p, k, s) for (p, k, s, _, _) in tz.MARGINS.worst}]
    worst = max(list(merged.worst.values()) + list(tz.MARGINS.worst.values()), default=0.0)
    share = max(ts.SHARES.values(), default=0.0)
    lines = ["certificate margins: python scripts/dev_certificates.py on one MI355X",
             "measured at commit %s" % commit,
             "tests/test_gpu_certificates.py, tests/test_gpu_sketch_state.py, tests/test_gpu_coincident.py: exit code %d; largest ratio %.4f; kinds without a margin: %s"
             % (int(rc), worst, missing or "none"),
             "ratio = the largest |key - real-number key| / (ub - key) over every key checked (bf16-operands: |key - the",
             "key of the emulated bfloat16 operands| / the float32-accumulation part of key_eps's bfloat16 branch)", ""]
    lines += merged.lines()
    lines += ["", "keys at and near zero (tests/test_gpu_coincident.py: queries on stored rows and within a few float32 spacings of",
              "them, 2 005 rows at the most; the requirement is max ratio <= 1 on every line)"]
    lines += tz.MARGINS.lines()
    lines += ["", "B3, the farthest row from its sketch as a share of the slack the search allows (1 - share shown: what is",
              "left; cosine slack carries the angles' rounding term, Euclidean slack only the factor 1 + 1e-9)",
              "%-6s %5s %12s" % ("metric", "dim", "1 - share")]
    lines += ["%-6s %5d %12.3e" % ("cosine" if m else "euclid", d, 1.0 - v) for (m, d), v in sorted(ts.SHARES.items())]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if rc or missing or worst > 1.0 or share > 1.0 else 0


if __name__ == "__main__":
    sys.exit(main())
