"""A short run of the differential fuzzer (scripts/fuzz_gpu.py): random shapes, masks,
tombstones, two-shard handles and tunables against the oracle."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Cases per seed: a fixed count, so a seed means the same cases on every run and every card.  The fuzzer's former
# 12-second budget ran 147 cases (seed 11) and 173 (seed 12) on an MI355X; the count is the larger one, rounded up.
# With the soaking options and the sketch sweep's forms among the tunables drawn (their own stream: every other draw of
# the two seeds is what it was), 180 cases take 14.4 s (seed 11) and 15.5 s (seed 12) on an MI355X.
FUZZ_ITERATIONS = 180


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 12])
def test_fuzz_short(seed):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_gpu.py"), "12", str(seed),
                        "--iterations", str(FUZZ_ITERATIONS)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "0 failures" in p.stdout


@pytest.mark.gpu
def test_collection_fuzz_short():
    """Stateful fuzz of the Collection mirror (add / re-add / remove / update / search / list)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_collection.py"), "10", "5"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "0 failures" in p.stdout
