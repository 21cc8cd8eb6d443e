"""szg_set_option on a live handle, held to the hand-written list of option_cases.py: codes, texts and -- read back
through szg_debug_option_get -- what is stored; and the forwarding rule: the internal sketch index follows 30 of the 36
options (those set before it exists are replayed when it is created, with their last values) and keeps its defaults of
the other six.  A float32 cosine handle of 300 rows x 32 in two shards on one device, sketch = 1, sketch_min_rows = 1.
An older build of the library (SZG_LIB_PATH) has no read-back hook: codes and texts are checked all the same."""
import os

import numpy as np
import pytest

import option_cases as oc
import oracle as orc
from syzgydb_amd import ScanIndex, SzgError, SZG_COSINE, _lib

pytestmark = pytest.mark.gpu
N, DIM = 300, 32
READ_BACK = hasattr(_lib.load(), "szg_debug_option_get")
needs_read_back = pytest.mark.skipif(not READ_BACK, reason="this build of the library has no szg_debug_option_get")

# a legal value that is not the default, for every option (LATER: set after those, for the two that are set twice)
OTHER = {"sketch_list": 12, "sketch_extra": 20, "force_sketch_nomem": 1, "carry_stage_bytes": 4096,
         "slack": 20, "queries_per_launch": 8, "scan_group": 2, "scan_group_ring": 4, "scan_norms": 1, "sketch_planes": 3,
         "sketch_matrix": 1, "sketch_select": 1, "sketch_wide": 1, "sketch_share": 1, "sketch_bulk": 1, "sketch_radius": 1,
         "sketch_masked": 1, "sketch_f64": 1, "sketch_topk_collect": 1, "query_prep": 1, "query_batch": 32, "radius_mq": 0,
         "finish_thread": 0, "contexts": 2, "multi_query": 0, "mask_dense": 0, "coalesce": 0, "force_matrix": 1,
         "force_no_refine": 1, "mq_hits": 2048, "mq_min": 3, "serialize_scans": 0, "tie_mode": 1, "force_escalate": 1}
LATER = {"scan_group": 1, "query_batch": 8}
SETUP = {"sketch": 1, "sketch_min_rows": 1}   # (the two of the six that the handle's setup sets)


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(20261)
    V = rng.standard_normal((N, DIM))
    rows = orc.encode_rows(V, 32)
    return rows, V.astype(np.float32).astype(np.float64), rng.standard_normal(DIM)


def open_handle(rows):
    ix = ScanIndex(DIM, 32, SZG_COSINE, devices=[0, 0])
    ix.load(rows)
    for name, value in SETUP.items():
        ix.set_option(name, value)
    return ix


def refused(ix, name, value, text):
    with pytest.raises(SzgError) as e:
        ix.set_option(name, value)
    assert e.value.code == _lib.SZG_E_INVALID and ("(%s)" % text) in str(e.value), (name, value, str(e.value))


def test_edges_and_read_back(corpus):
    with open_handle(corpus[0]) as ix:
        for name, case in oc.CASES.items():
            held = ix.debug_option(name) if READ_BACK else None
            for value in case["refused"]:
                refused(ix, name, value, case["text"])
                if READ_BACK:
                    assert ix.debug_option(name) == held, (name, value)
            for value, stored in case["accepted"]:
                ix.set_option(name, value)
                if READ_BACK:
                    assert ix.debug_option(name) == stored, (name, value)
                for bad in case["refused"][:1]:   # a refusal leaves the value from before
                    refused(ix, name, bad, case["text"])
                    if READ_BACK:
                        assert ix.debug_option(name) == stored, (name, value, bad)


@needs_read_back
def test_defaults(corpus):
    preset = {item.split("=")[0].strip() for item in os.environ.get("SZG_OPTIONS", "").split(",")}   # (set on every new handle)
    with ScanIndex(DIM, 32, SZG_COSINE, devices=[0, 0]) as ix:
        for name, case in oc.CASES.items():
            if name not in preset:
                assert ix.debug_option(name) == case["default"], name


def brute_force(V, q, k):
    cos = (V @ q) / (np.linalg.norm(V, axis=1) * np.linalg.norm(q))
    return [int(i) for i in np.argsort(-cos, kind="stable")[:k]]


@needs_read_back
def test_replay_at_sketch_creation(corpus):
    rows, V, q = corpus
    with open_handle(rows) as ix:
        for name in oc.CASES:
            with pytest.raises(SzgError) as e:
                ix.debug_option(name, on_sketch=True)
            assert e.value.code == _lib.SZG_E_UNSUPPORTED
        assert set(OTHER) | set(SETUP) == set(oc.CASES)
        for name, value in OTHER.items():
            assert value != oc.CASES[name]["default"]
            ix.set_option(name, value)
        for name, value in LATER.items():
            assert name in oc.FORWARDED and value not in (OTHER[name], oc.CASES[name]["default"])
            ix.set_option(name, value)
        last = dict(OTHER, **LATER)
        ix.set_option("force_sketch_nomem", 0)   # (the hook would refuse the sketch its memory: non-default until here)
        r, d, c = ix.search_topk(q[None, :], 3)
        assert c[0] == 3 and [int(x) for x in r[0]] == brute_force(V, q, 3)
        o_rows, o_dist, _ = orc.search_exact(rows, DIM, 32, SZG_COSINE, q, k=3)
        assert [int(x) for x in r[0]] == [int(x) for x in o_rows] and (d[0] == o_dist).all()
        for name in oc.FORWARDED:
            assert ix.debug_option(name, on_sketch=True) == last[name], name
            assert ix.debug_option(name) == last[name], name
        for name in oc.NOT_FORWARDED:
            assert ix.debug_option(name, on_sketch=True) == oc.CASES[name]["default"], name


@needs_read_back
def test_forwarding_to_an_existing_sketch(corpus):
    rows, V, q = corpus
    with open_handle(rows) as ix:
        ix.set_option("multi_query", 0)
        r, _, _ = ix.search_topk(q[None, :], 3)
        assert [int(x) for x in r[0]] == brute_force(V, q, 3)
        for name in oc.FORWARDED:
            case = oc.CASES[name]
            for value in (OTHER[name], case["accepted"][0][0]):
                stored = dict(case["accepted"]).get(value, value)
                ix.set_option(name, value)
                assert (ix.debug_option(name), ix.debug_option(name, on_sketch=True)) == (stored, stored), (name, value)
            for bad in case["refused"]:
                refused(ix, name, bad, case["text"])
                assert (ix.debug_option(name), ix.debug_option(name, on_sketch=True)) == (stored, stored), (name, bad)
        for name in oc.NOT_FORWARDED:
            case = oc.CASES[name]
            on_sketch = ix.debug_option(name, on_sketch=True)
            value = OTHER.get(name, case["accepted"][0][0] + 1)   # ("sketch": 1, "sketch_min_rows": 2)
            ix.set_option(name, value)
            assert ix.debug_option(name) == value != on_sketch, name
            assert ix.debug_option(name, on_sketch=True) == on_sketch, name
            for bad in case["refused"]:
                refused(ix, name, bad, case["text"])
                assert (ix.debug_option(name), ix.debug_option(name, on_sketch=True)) == (value, on_sketch), (name, bad)


def test_error_texts(corpus):
    L = _lib.load()
    with open_handle(corpus[0]) as ix:
        for name in ("nonsense", "", "slack_min", "sketch_on", "Sketch"):
            refused(ix, name, 1, "unknown option")
        assert L.szg_set_option(ix._h, None, 1) == _lib.SZG_E_INVALID and L.szg_last_error() == b"null argument"
        if READ_BACK:
            with pytest.raises(SzgError) as e:
                ix.debug_option("nonsense")
            assert e.value.code == _lib.SZG_E_INVALID and "(unknown option)" in str(e.value)
    assert L.szg_set_option(None, b"slack", 1) == _lib.SZG_E_INVALID and L.szg_last_error() == b"null argument"
