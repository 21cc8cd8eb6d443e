"""Option "contexts" on a handle that has already served searches.  A call with one sweep per query borrows only a
shard's lowest-numbered contexts (one stream per hardware queue), and contexts come back to the
free list in the order their batches finish -- so the option must park by context number, not by position in that list,
or a later one-sweep call finds no context it may take and waits forever."""
import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import ScanIndex, SZG_COSINE

pytestmark = pytest.mark.gpu


def same(a, b):
    (ra, da, ca), (rb, db, cb) = a, b
    assert (ca == cb).all()
    for qi in range(len(ca)):
        n = ca[qi]
        assert (ra[qi, :n] == rb[qi, :n]).all(), qi
        assert (da[qi, :n].view(np.uint64) == db[qi, :n].view(np.uint64)).all(), qi


@pytest.mark.parametrize("bits,sketch", [(8, 0), (32, 1)], ids=["plain-8bit", "float32-sketch"])
def test_contexts_after_multi_batch_one_sweep_calls(bits, sketch):
    dim, n, k = 64, 20000, 10
    rows = orc.synth_rows(0x5A01 + bits, 0, n, dim, bits)
    Q = orc.synth_vectors(0x5A02, 0, 150, dim)
    with ScanIndex(dim, bits, SZG_COSINE) as ix:
        ix.load(rows)
        for name, v in (("multi_query", 0), ("sketch", sketch), ("sketch_min_rows", 1)):
            ix.set_option(name, v)
        want = ix.search_topk(Q, k)           # many batches: every context in rotation is used and returned
        o_rows, o_dist, _ = orc.search_exact(rows, dim, bits, SZG_COSINE, Q[7], k=k)
        assert [int(x) for x in want[0][7, :k]] == [int(x) for x in o_rows] and (want[1][7, :k] == o_dist).all()
        for contexts in (1, 2, 3, 4, 2, 1, 3):
            ix.set_option("contexts", contexts)
            same(ix.search_topk(Q, k), want)          # a long call: batches queue for the contexts left
            same(ix.search_topk(Q[:5], k), tuple(x[:5] for x in want))   # a short call: one batch
            ix.search_topk(Q[:40], k)                 # leave the free list in another order for the next setting
        ix.set_option("multi_query", 1)               # shared sweeps take every context in rotation
        ix.set_option("contexts", 1)
        got = ix.search_topk(Q, k)
        assert (got[0] == want[0]).all()
