"""The pinned runs of the stateful fuzzer (scripts/fuzz_state.py): one handle per case under mutations, masks, columns,
readers and searches, every answer the oracle's -- and the `served` counters show that the runs reached the paths the
fuzzer exists for."""
import json
import subprocess

import pytest

import fuzz_state_pins as pins

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("profile,seed", pins.PINS)
def test_fuzz_state(profile, seed):
    p = subprocess.run(pins.command(profile, seed), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-6000:] + p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out["served"]))
    assert out["cases"] == pins.CASES and out["failures"] == 0
    # the card ran the plan that --plan-only prints (and tests/test_fuzz_state_cpu.py holds to its coverage): the same
    # operation log, case by case, and the same counts -- no draw of the generator depends on the card
    q = subprocess.run(pins.command(profile, seed, "--plan-only"), capture_output=True, text=True, timeout=300)
    assert q.returncode == 0, q.stdout[-3000:] + q.stderr[-2000:]
    plan = json.loads(q.stdout.strip().splitlines()[-1])
    assert out["plan"] == plan["plan"] and out["operations"] == plan["operations"]
    served, ops = out["served"], out["operations"]
    if profile == "plain":
        assert served["mq_queries"] > 0 and served["mq_bf16_sweeps"] > 0
        missing = [k for k in pins.fuzz_state.KINDS if ops.get(k, 0) == 0]
        assert not missing, missing
    else:
        assert served["sketch_queries"] > 0
        assert served["sketch_radius_queries"] > 0
        assert served["sketch_topk_collect_queries"] > 0
        assert served["sketch_masked_launches"] > 0
        assert served["sketch_queries_64bit"] > 0
