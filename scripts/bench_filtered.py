"""Filtered top-k on the headline corpus (1M x 768, 32-bit, cosine, k = 10, synthesised on the device): what a filter
costs per query when it arrives as allow_bits words with every call, as ONE resident mask shared by all queries, or
as a resident mask per query.

Legs: selectivity 5 % and 0.1 % x {one query per call, one 96-query call} x {words, shared handle, 96 distinct
handles}.  Per leg: a warm-up region, then value = the MEDIAN of 5 timed regions in queries/s, spread = min / max,
and the szg_mask_stats deltas of the timed regions.  One JSON line on stdout.

The words legs use only the allow_bits API, so they also run against an older build of the library selected
through SZG_LIB_PATH (the handle legs are skipped there): run both builds in ONE job, on one box.
SZG_ROWS / SZG_REGIONS / SZG_CALLS (single-query calls per region, 32) shrink it for a rehearsal."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syzgydb_amd import ScanIndex, _lib, pack_allow_bits  # noqa: E402
from syzgydb_amd.synth import synth_vectors  # noqa: E402

DIM, BITS, METRIC, K, NQ = 768, 32, 1, 10, 96
N = int(os.environ.get("SZG_ROWS", "1000000"))
REGIONS = int(os.environ.get("SZG_REGIONS", "5"))
CALLS = int(os.environ.get("SZG_CALLS", "32"))


def region(ix, mode, kind, Q, words, handles):
    """One timed region: CALLS single-query calls, or one NQ-query call.  Returns (seconds, queries)."""
    if mode == "single":
        t0 = time.perf_counter()
        for i in range(CALLS):
            j = i % NQ
            if kind == "words":
                ix.search_topk(Q[j], K, allow=words[0 if words.shape[0] == 1 else j][None, :])
            else:
                ix.search_topk(Q[j], K, masks=handles[0 if len(handles) == 1 else j])
        return time.perf_counter() - t0, CALLS
    t0 = time.perf_counter()
    if kind == "words":
        ix.search_topk(Q, K, allow=words if words.shape[0] == NQ else np.repeat(words, NQ, axis=0))
    else:
        ix.search_topk(Q, K, masks=handles[0] if len(handles) == 1 else handles)
    return time.perf_counter() - t0, NQ


def main():
    L = _lib.load()
    has_masks = hasattr(L, "szg_mask_create")
    rng = np.random.default_rng(7)
    legs = []
    with ScanIndex(DIM, BITS, METRIC, devices=[0]) as ix:
        ix.synth(N, 1234)
        ix.search_topk(synth_vectors(98, 0, 1, DIM)[0], K)  # builds the sketch: not part of any leg
        for sel in (0.05, 0.001):
            words = np.concatenate([pack_allow_bits(rng.random(N) < sel) for _ in range(NQ)])
            shared = [ix.mask(words[:1])] if has_masks else None
            distinct = [ix.mask(words[j:j + 1]) for j in range(NQ)] if has_masks else None
            for mode in ("single", "batch"):
                for kind, w, h in (("words", words[:1], None), ("words_distinct", words, None),
                                   ("shared_handle", None, shared), ("distinct_handles", None, distinct)):
                    if kind.endswith(("handle", "handles")) and not has_masks:
                        continue
                    api = "words" if kind.startswith("words") else "handles"
                    Q = synth_vectors(100 + len(legs), 0, NQ * (REGIONS + 1), DIM)
                    region(ix, mode, api, Q[:NQ], w, h)  # warm-up: every shape the timed regions use
                    before = ix.mask_stats() if has_masks else None
                    rates = []
                    for r in range(REGIONS):
                        sec, n = region(ix, mode, api, Q[NQ * (r + 1):NQ * (r + 2)], w, h)
                        rates.append(n / sec)
                    leg = {"selectivity": sel, "call": "1 query" if mode == "single" else "%d queries" % NQ, "filter": kind,
                           "value": round(float(np.median(rates)), 1), "unit": "queries/s",
                           "spread": {"min": round(min(rates), 1), "max": round(max(rates), 1), "repeats": REGIONS}}
                    if has_masks:
                        after = ix.mask_stats()
                        leg["mask_stats"] = {key: after[key] - before[key] for key in ("h2d_bytes", "d2d_bytes", "shared_batches")}
                    legs.append(leg)
            for m in (shared or []) + (distinct or []):
                m.close()
    print(json.dumps({"bench": "filtered_topk", "library": _lib.LIB_PATH, "handles": has_masks,
                      "corpus": {"rows": N, "dim": DIM, "bits": BITS, "metric": "cosine", "k": K},
                      "calls_per_region": {"1 query": CALLS, "%d queries" % NQ: 1}, "legs": legs}))


if __name__ == "__main__":
    main()
