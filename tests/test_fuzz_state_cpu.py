"""scripts/fuzz_state.py without a card: its plan is a function of the seed, the pinned runs draw everything the fuzzer
exists for, and its checkers flag what they are for.  No device is touched: --plan-only runs the generator, the model and
the oracle alone."""
import functools
import json
import subprocess

import numpy as np
import pytest

import fuzz_state_pins as pins

fz = pins.fuzz_state
DTYPES = ("f64", "f32", "f16", "bf16")
TENSOR_ENTRIES = ("append_tensor", "overwrite_tensor", "search_topk_tensor", "search_radius_tensor", "fetch_range", "fetch_list")


@functools.lru_cache(maxsize=None)
def plan(profile, seed, cases=pins.CASES):
    cmd = pins.command(profile, seed, "--plan-only")
    cmd[cmd.index("--cases") + 1] = str(cases)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    return p.stdout


def counts(profile, seed):
    return json.loads(plan(profile, seed).strip().splitlines()[-1])["operations"]


# ---- the plan is a function of the seed ------------------------------------------------------------------------------------
def test_the_same_seed_gives_the_same_plan_and_another_seed_another():
    plan.cache_clear()
    first = plan("sketched", 31, 10)
    plan.cache_clear()
    assert plan("sketched", 31, 10) == first
    assert len(json.loads(first.strip().splitlines()[-1])["plan"]) == 64   # the digest the card run is compared by
    assert plan("sketched", 31, 12).startswith(first[: first.rindex("CASE ")])   # a case's plan does not depend on the count
    assert first.count("CASE ") == 10 and "search_topk" in first
    assert plan("sketched", 32, 10) != first
    assert plan("plain", 31, 10) != first


# ---- what the pinned runs draw -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile,seed", pins.PINS)
def test_every_operation_kind_is_drawn(profile, seed):
    ops = counts(profile, seed)
    few = {k: ops.get(k, 0) for k in fz.KINDS + ["option_redraw"] + ["where:%s" % op for op in fz.CMP] if ops.get(k, 0) < 3}
    assert not few, few
    assert ops["base:with"] >= 3 and ops["base:without"] >= 3
    assert ops["allow:words"] >= 3 and ops["allow:bool"] >= 3   # host filters as the caller's words and as booleans
    assert ops["col_new:f64"] >= 3 and ops["col_new:text"] >= 3


@pytest.mark.parametrize("profile,seed", pins.PINS)
def test_every_dtype_of_every_tensor_entry_point_is_drawn(profile, seed):
    ops = counts(profile, seed)
    few = {"%s:%s" % (e, d): ops.get("%s:%s" % (e, d), 0) for e in TENSOR_ENTRIES for d in DTYPES if ops.get("%s:%s" % (e, d), 0) < 3}
    assert not few, few


@pytest.mark.parametrize("profile,seed", pins.PINS)
def test_shards_and_widths(profile, seed):
    ops = counts(profile, seed)
    assert ops.get("shards:1", 0) >= 3 and ops.get("shards:2", 0) >= 3
    for bits in ((32, 64) if profile == "sketched" else (4, 8, 16, 32, 64)):
        assert ops.get("bits:%d" % bits, 0) >= 3, bits


@pytest.mark.parametrize("profile,seed", [p for p in pins.PINS if p[0] == "sketched"])
def test_the_soaking_options_meet_the_calls_they_change(profile, seed):
    ops = counts(profile, seed)
    for name in ("sketch_masked", "sketch_radius", "sketch_f64", "sketch_topk_collect"):
        assert ops.get("option:%s" % name, 0) >= 5, name
    assert ops.get("coincide:sketch_masked", 0) >= 3         # sketch_masked = 1 and a filtered or tombstoned top-k
    assert ops.get("coincide:sketch_topk_collect", 0) >= 3   # sketch_topk_collect = 1, a served sample plan and k >= 35


# ---- the checkers catch what they are for ----------------------------------------------------------------------------------
ROWS = np.array([7, 3, 11, 0, 5], dtype=np.uint64)
DIST = np.array([0.0, 0.25, 0.5, np.nan, np.nan])
LIVE = np.ones(12, dtype=bool)


def test_same_answer():
    assert fz.same_answer(ROWS.copy(), DIST.copy(), ROWS, DIST, live=LIVE)
    assert fz.same_answer(ROWS + np.uint64(1000), DIST.copy(), ROWS + np.uint64(1000), DIST, live=LIVE, base=1000)
    swapped = ROWS.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    assert not fz.same_answer(swapped, DIST, ROWS, DIST)                      # two adjacent rows swapped
    ulp = DIST.copy()
    ulp[1] = np.nextafter(ulp[1], 1.0)
    assert not fz.same_answer(ROWS, ulp, ROWS, DIST)                          # a distance one ulp off
    dead = LIVE.copy()
    dead[11] = False
    assert not fz.same_answer(ROWS, DIST, ROWS, DIST, live=dead)              # a tombstoned row among the hits
    assert not fz.same_answer(ROWS[:-1], DIST[:-1], ROWS, DIST)               # a missing last hit
    number = DIST.copy()
    number[3] = 0.75
    assert not fz.same_answer(ROWS, number, ROWS, DIST)                       # a NaN paired with a number
    assert not fz.same_answer(ROWS, DIST, ROWS, number)
    minus = DIST.copy()
    minus[0] = -0.0
    assert not fz.same_answer(ROWS, minus, ROWS, DIST)                        # equal, but not on the bits
    assert not fz.same_answer(ROWS, DIST, ROWS, DIST, live=LIVE, base=1)      # a row below the base


def test_same_rows():
    want = np.arange(60, dtype=np.uint8).reshape(5, 12)
    assert fz.same_rows(want.copy(), want)
    off = want.copy()
    off[4, 11] ^= 1
    assert not fz.same_rows(off, want)
    assert not fz.same_rows(want[:4], want)


def test_same_mask():
    want = np.zeros(70, dtype=bool)
    want[[0, 63, 64, 69]] = True
    words = fz.pack_bits(want)
    assert words.size == 2 and int(words[1]) == 0b100001
    assert fz.same_mask(words.copy(), want)
    for bit in (5, 6, 63):   # a row of the tail word; the first bit past the rows; the last bit of the word
        off = words.copy()
        off[1] ^= np.uint64(1) << np.uint64(bit)
        assert not fz.same_mask(off, want), bit
    assert not fz.same_mask(words[:1], want)


def test_same_column():
    vals = np.array([1.5, np.nan, -0.0, 3.0])
    pres = np.array([True, True, True, False])
    assert fz.same_column(vals.copy(), pres.copy(), vals, pres)
    other = vals.copy()
    other[3] = 99.0   # an absent row's value is nobody's business
    assert fz.same_column(other, pres, vals, pres)
    flipped = pres.copy()
    flipped[0] = False
    assert not fz.same_column(vals, flipped, vals, pres)                      # the value equal, the present bit not
    flipped = pres.copy()
    flipped[3] = True
    assert not fz.same_column(vals, flipped, vals, pres)
    zero = vals.copy()
    zero[2] = 0.0
    assert not fz.same_column(zero, pres, vals, pres)                         # +0.0 for -0.0
    text = [b"ab", b"", b"a\x00", b"zz"]
    assert fz.same_column(list(text), pres, text, pres)
    assert not fz.same_column([b"ab", b"", b"a", b"zz"], pres, text, pres)
    assert not fz.same_column(list(text), flipped, text, pres)


def test_same_tensor_bits():
    for dtype in (np.float64, np.float32, np.float16):
        want = np.array([[0.0, -0.0, 1.5], [np.nan, -2.0, np.inf]], dtype=dtype)
        assert fz.same_tensor_bits(want.copy(), want)
        off = want.copy()
        off[0, 0] = -0.0
        assert not fz.same_tensor_bits(off, want), dtype                      # -0.0 against +0.0: the bits differ
        off = want.copy()
        off[1, 0] = 1.0
        assert not fz.same_tensor_bits(off, want)
        assert not fz.same_tensor_bits(want.astype(np.float64 if dtype != np.float64 else np.float32), want)
    bf = np.array([0x0000, 0x8000, 0x3FC0, 0x7FC0], dtype=np.uint16)          # bfloat16 as bits: 0, -0, 1.5, NaN
    assert fz.same_tensor_bits(bf.copy(), bf)
    assert fz.same_tensor_bits(np.array([0, 0x8000, 0x3FC0, 0x7FC1], dtype=np.uint16), bf)   # NaNs are equal
    assert not fz.same_tensor_bits(np.array([0x8000, 0x8000, 0x3FC0, 0x7FC0], dtype=np.uint16), bf)


def test_round_to_is_exact_in_the_type():
    import torch
    v = np.random.default_rng(5).uniform(-1.25, 1.25, 4000)
    v[:6] = [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9 + 2.0 ** -30, 3.0e-8]   # bfloat16 ties
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        got = fz.round_to(v, name)
        if name in ("f32", "bf16"):   # (nearest even, as torch rounds)
            assert (got == torch.from_numpy(v).float().to(dtype).double().numpy()).all(), name
        assert (torch.from_numpy(got).to(dtype).double().numpy() == got).all(), name   # the tensor holds these very values
    assert (fz.round_to(v, "f64") == v).all()
