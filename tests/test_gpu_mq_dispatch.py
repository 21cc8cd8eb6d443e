"""Every arm of the shared sweeps' host dispatch (kernels_mq.hip and the family sources behind it), at the bar of
test_gpu_multiquery.py: ids identical to the oracle's, float64 distances bit-equal.

One case = one row width and metric.  It walks every query-block count of the width's family (nq = 16 nb - 3), each
through the fused selection (threshold pass + collecting sweep) and through the score matrix (force_matrix), a radius
batch (the collect arm on its own), a dimension of whole 64-byte steps and a ragged one (the predicate-free and the
predicated int8 kernel), the three row shapes with an int8 kernel of their own, and one dimension whose image no
longer fits LDS with the blocks the batch asks for.  Shapes are the smallest that reach each arm."""
import os

import numpy as np
import pytest

import oracle as orc
from syzgydb_amd import ScanIndex, SZG_COSINE, SZG_EUCLIDEAN

pytestmark = pytest.mark.gpu

# statistics of a particular path are asserted only under the default tunables (see test_gpu_multiquery.py)
DEFAULT_TUNABLES = not os.environ.get("SZG_OPTIONS")
# ... and for 8-bit rows only without the two hooks that move them between the int8 and the bfloat16 sweep
DEFAULT_8BIT = not os.environ.get("SZG_BF16_8BIT") and not os.environ.get("SZG_NO_ROW_NORMS")

K = 5            # kp = 21: the threshold pass takes 16 kp = 336 rows, and a shard of >= 4 x 336 = 1 344 rows is swept fused
N_ROWS = 2000    # (scan_mq.cpp: mq_plan)
N_ROWS_LDS = 600


def cdiv(a, b):
    return -(-a // b)


def r16_of(bits, dim):
    return cdiv(cdiv(dim * bits, 8), 16)     # 16-byte pieces per row


def takes_bf16(bits, dim, nq):
    """The bfloat16 sweeps: 16-, 32- and 64-bit rows, and top-k batches of more than 48 queries on 8-bit rows of whole
    64-byte steps (scan_query.cpp: mq_uses_bf16)."""
    return bits >= 16 or (bits == 8 and nq > 48 and r16_of(bits, dim) % 4 == 0)


def bf16_lds_bytes(bits, r16, nb):   # kernels_mq.hip: mq_bf16_lds_bytes (a KiB per 32-element K-step and query block)
    if bits == 8:
        ksteps = cdiv(r16, 4) * 2
    else:
        steps = cdiv(r16, 8)
        ksteps = cdiv(steps, 2) if bits == 64 else steps * (2 if bits == 16 else 1)
    return ksteps * nb * 1024 + 3 * 96 * 4 + max(8 * (64 * 9 + 1024), 12 * 64 * 9)


def i8_lds_bytes(bits, r16, nb, groups=1):   # kernels_mq.hip: mq_i8_lds_bytes (two digit planes, 4-bit rows: two nibble halves)
    return groups * (cdiv(r16, 4) * 2 * (2 if bits == 4 else 1) * nb * 1024 + 6 * 48 * 4) + 12 * 64 * 9


def blocks(bits, dim, nq):
    """scan_query.cpp: mq_blocks -- the query blocks of 16 a batch gets: what it asks for, capped by its family (6 / 3)
    and by what fits LDS (the published limits: 160 KiB for the bfloat16 image, 150 KiB for the int8 one)."""
    bf16, r16 = takes_bf16(bits, dim, nq), r16_of(bits, dim)
    nb = min(cdiv(nq, 16), 6 if bf16 else 3)
    while nb > 0 and (bf16_lds_bytes(bits, r16, nb) > 160 * 1024 if bf16 else i8_lds_bytes(bits, r16, nb) > 150 * 1024):
        nb -= 1
    return nb


def launches(bits, dim, nq):
    """Sweep launches of one top-k call of nq queries (scan_topk.cpp: plan_batch): batches of 16 nb queries, the int8
    sweeps walking two groups of 48 (counted as two) where both images fit."""
    left, n = nq, 0
    while left >= 2:
        nb = blocks(bits, dim, left)
        assert nb > 0
        if takes_bf16(bits, dim, left):
            take, n = min(left, 16 * nb), n + 1
        else:
            two = nb == 3 and left > 48 and i8_lds_bytes(bits, r16_of(bits, dim), 3, 2) <= 160 * 1024
            take = min(left, 16 * nb * (2 if two else 1))
            n += cdiv(take, 16 * nb)
        left -= take
    assert left == 0   # (a single query left over would get a sweep of its own: the cases below avoid that)
    return n


def lds_limited_dim(bits, nq):
    """The smallest dimension at which the image of ceil(nq / 16) query blocks no longer fits LDS."""
    dim = 1
    while blocks(bits, dim, nq) == min(cdiv(nq, 16), 6 if takes_bf16(bits, dim, nq) else 3):
        dim += 1
    return dim


class Corpus:
    """Rows, 93 queries and the oracle's answers, computed once per (width, metric, dim, rows) and never changed."""
    _cache = {}

    def __init__(self, bits, metric, dim, n, nq):
        self.bits, self.metric, self.dim, self.n = bits, metric, dim, n
        self.rows = orc.synth_rows(5100 + dim + bits, 0, n, dim, bits)
        self.Q = orc.synth_vectors(5101 + dim + bits, 0, nq, dim)
        self.top = [orc.search_exact(self.rows, dim, bits, metric, q, k=K)[:2] for q in self.Q]

    @classmethod
    def get(cls, bits, metric, dim, n, nq=93):
        key = (bits, metric, dim, n, nq)
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def check_topk(self, ix, nq, want_launches=None):
        ix.reset_stats()
        r, d, c = ix.search_topk(self.Q[:nq], K)
        for qi in range(nq):
            o_rows, o_dist = self.top[qi]
            assert c[qi] == len(o_rows), (nq, qi)
            assert [int(x) for x in r[qi, : c[qi]]] == [int(x) for x in o_rows], (nq, qi)
            assert (d[qi, : c[qi]] == o_dist).all(), (nq, qi)
        if want_launches is not None and DEFAULT_TUNABLES and (self.bits != 8 or DEFAULT_8BIT):
            st = ix.stats()
            assert (st["mq_queries"], st["mq_launches"]) == (nq, want_launches), (nq, st)

    def check_radius(self, ix, nq):
        radii = [float(self.top[qi][1][-1]) for qi in range(nq)]   # the K-th distance: K rows or a few more (ties)
        hits = ix.search_radius_batch(self.Q[:nq], radii)
        for qi in range(nq):
            w_r, w_d, _ = orc.search_exact(self.rows, self.dim, self.bits, self.metric, self.Q[qi], radius=radii[qi])
            assert [int(x) for x in hits[qi][0]] == [int(x) for x in w_r], qi
            assert (np.asarray(hits[qi][1]) == w_d).all(), qi


@pytest.mark.parametrize("metric", [SZG_COSINE, SZG_EUCLIDEAN])
@pytest.mark.parametrize("bits", [4, 8, 16, 32, 64])
def test_every_dispatch_arm(bits, metric):
    max_nb = 3 if bits == 4 else 6   # (8-bit rows: nb 1..3 are the int8 sweep, 4..6 -- more than 48 queries -- the bfloat16 one)
    # whole 64-byte steps and a ragged row.  (64 4-bit codes are half a step: 128 is what reaches the predicate-free
    # int8 kernel on 4-bit rows.)
    for dim in (64, 37) + ((128,) if bits == 4 else ()):
        cp = Corpus.get(bits, metric, dim, N_ROWS)
        with ScanIndex(dim, bits, metric) as ix:
            ix.load(cp.rows)
            for force_matrix in (0, 1):   # the fused selection (N_ROWS >= 1 344), then the score matrix
                ix.set_option("force_matrix", force_matrix)
                for nb in range(1, max_nb + 1):
                    nq = 16 * nb - 3
                    assert blocks(bits, dim, nq) == min(nb, 6 if takes_bf16(bits, dim, nq) else 3)
                    cp.check_topk(ix, nq, launches(bits, dim, nq))
            ix.set_option("force_matrix", 0)
            cp.check_radius(ix, 20)       # the collect arm: the radius is the threshold, no threshold pass
    if bits in (4, 8):
        # 12, 6 and 3 64-byte steps per row: the shapes with an int8 kernel of their own, taken by full groups (NB == 3).
        # (4-bit rows of 1 536 dims: the image of three blocks does not fit LDS, the batch goes as 32 + 8 queries.)
        for dim in ((192, 384, 768) if bits == 8 else (384, 768, 1536)):
            assert r16_of(bits, dim) // 4 in (3, 6, 12) and r16_of(bits, dim) % 4 == 0
            cp = Corpus.get(bits, metric, dim, N_ROWS, 40)
            with ScanIndex(dim, bits, metric) as ix:
                ix.load(cp.rows)
                cp.check_topk(ix, 40, launches(bits, dim, 40))
    # the image of the blocks the batch asks for does not fit LDS: fewer blocks per sweep, more sweeps.  With the full
    # batch of each family (93 queries = 6 blocks, 45 = 3 on the int8 sweeps) the smallest such dimensions are
    #   769 for 32-, 16- and 64-bit rows (25 K-steps x 6 KiB + 13.6 KiB of tables, hit buffers and staging > 160 KiB),
    #   1 473 for 8-bit rows (24 steps x 6 KiB + 7.9 KiB > 150 KiB) and 1 409 for 4-bit rows (12 steps x 12 KiB + 7.9 KiB)
    nq = 93 if bits >= 16 else 45
    dim = lds_limited_dim(bits, nq)
    assert dim == {32: 769, 16: 769, 64: 769, 8: 1473, 4: 1409}[bits]
    assert blocks(bits, dim, nq) == cdiv(nq, 16) - 1 and launches(bits, dim, nq) == 2
    cp = Corpus.get(bits, metric, dim, N_ROWS_LDS, nq)
    with ScanIndex(dim, bits, metric) as ix:
        ix.load(cp.rows)
        cp.check_topk(ix, nq, 2)
