"""The masked long-row forms of the matrix sketch sweep (kernels_scan_mx.hip -DSZG_MX_LONG -DSZG_MX_MASKED; sketch_masked = 1
at 1 920, 2 048 and 4 096 dimensions) on the corpora, lists of 12 and forced wide / shared launches of test_gpu_sketch_long.
One leg of test_gpu_sketch_masked per case, the plan hook's passes (off: one per query, which differs modulo 4 at every
call size here), and no more queries handed over than with the option off.  T tiles of 16 rows, a wave walks w, w + S, ...:
 tomb    a run of T / 4 dead tiles (waves lose a tile in mid-walk, or their only one), the tile before the ragged last
         one, every 97th row;
 shared  one resident mask: every 17th tile (5.9 %), tile 40 with its row 15 alone, no tile of wave 5, the last tile;
 perq    a resident mask per query at half the rows; half of tiles 7, 27 and 47 is query 2's alone, which has nothing
         else; query 1 has 7 rows.
Checked on the CPU when SALT was chosen (float64 distances, both metrics, every case): the lists of 12 keep every one of a
query's 44 best eligible rows (the sweeps' candidates are merged down to k + 30 = 40)."""
import numpy as np
import pytest

from syzgydb_amd import cert_check as cc
from syzgydb_amd.index import scan_long_plan, scan_plan
import test_gpu_sketch_long as tgl
import test_gpu_sketch_masked as tgm
import test_gpu_sketch_matrix as tsm

pytestmark = pytest.mark.gpu

K, LIST = tgl.K, tgl.LIST
GEOM = sorted([(1920, "s2", 16, 0), (2048, "s2", 16, 0), (2048, "s2", 16, 1), (4096, "s2", 16, 0), (4096, "s2", 16, 1)] +
              [(dim, "2999", nq, 0) for dim in (1920, 2048) for nq in (19, 37, 64)])   # (one corpus at a time)
SALT = {(1920, "s2"): 0, (2048, "s2"): 0, (4096, "s2"): 0, (1920, "2999"): 7, (2048, "2999"): 7}   # (the CPU check's choice)
PARAMS = [(g, kind, m) for g in GEOM for m in (tsm.COS, tsm.EUC) for kind in ("shared", "perq", "tomb")]


def wave_stride(dim, n, nq):
    """Tiles between two tiles of one wave: the grid (halved by blocks of 512, and by a shared launch's pairs) x waves."""
    g, p = scan_plan(dim, 8, n, kp=tsm.sketch_kp(K)), scan_long_plan(dim, 8, nq, kp=LIST)
    grid = -(-g["grid"] // 2) if p["block"] == 512 else g["grid"]
    return (max(1, grid // 2) if p["share"] else grid) * (p["block"] // 64)


def eligibility(kind, dim, rows, n, nq, stride):
    T, rng = -(-n // 16), np.random.default_rng(n + nq + 1000 * SALT[dim, rows])
    if kind == "tomb":
        ok, first = np.ones(T, dtype=bool), int(rng.integers(T - T // 4 - 2))
        ok[first: first + T // 4] = ok[T - 2] = False
        el = np.repeat(ok, 16)[:n]
        el[::97] = False
    elif kind == "shared":
        ok = np.arange(T) % 17 == int(rng.integers(17))
        ok[5::stride], ok[40], ok[T - 1] = False, False, True
        el = np.repeat(ok, 16)[:n]
        el[40 * 16 + 15] = True
    else:
        el = rng.random((nq, n)) < 0.5
        own = np.concatenate([np.arange(16 * t, 16 * t + 8) for t in (7, 27, 47)])   # (three block lists in every geometry)
        el[:, 7 * 16: 8 * 16] = el[:, 27 * 16: 28 * 16] = el[:, 47 * 16: 48 * 16] = el[1] = el[2] = False
        el[2, own] = True
        el[1, 48 * 16 + rng.choice(n - 48 * 16, 7, replace=False)] = True
    return el


@pytest.mark.parametrize("geom,kind,metric", PARAMS, ids=["d%d-n%s-q%d-s%d-" % g + kind + "-" + tsm.MID[m] for g, kind, m in PARAMS])
def test_masked_long_leg(geom, kind, metric):
    dim, rows, nq, select = geom
    packed, Qall, seed = tgl.data(dim, rows)
    n, Q, skip = packed.shape[0], Qall[:nq], kind != "perq"
    what = ("long rows, masked", geom, kind, tsm.MID[metric])
    plans = [scan_long_plan(dim, 8, c, kp=LIST, masked=True, sketch_masked=1, shared_mask=skip)
             for c in ([nq] if nq > 16 else tsm.launch_sizes(nq))]
    assert all(p["serves"] and p["tile_skip"] == skip for p in plans), (what, plans)
    assert plans[0]["blocks"] == (2 if nq > 16 else 1) and plans[0]["share"] == (nq > 32), (what, plans)
    el = eligibility(kind, dim, rows, n, nq, wave_stride(dim, n, nq))
    with tgm.open_masked(dim, metric, devices=[0], sketch_wide=2, sketch_share=2, sketch_list=LIST, sketch_select=select) as ix:
        ix.load(packed) if seed is None else ix.synth(n, seed)
        masks = [ix.mask(e) for e in el] if kind == "perq" else ([ix.mask(el)] if kind == "shared" else [])
        if kind == "tomb":
            ix.tombstone_rows(np.flatnonzero(~el))
        filt = {"masks": masks if kind == "perq" else masks[0]} if masks else {}
        try:
            # (eligibility per query in every kind: certified()'s chain that keeps no totals per dimension)
            tgm.leg(ix, cc.Corpus(packed, dim, 32, metric), Q, K, what, np.broadcast_to(el, (nq, n)), sum(p["passes"] for p in plans),
                    skip, **filt)
            handed = {}
            for opt in (1, 0):   # fallbacks are a condition: no more queries handed over than by the one-query kernel
                ix.set_option("sketch_masked", opt), ix.reset_stats(), ix.search_topk(Q, K, **filt)
                handed[opt] = ix.stats()["sketch_fallbacks"]
            assert handed[1] <= handed[0], (what, handed)
        finally:
            [m.close() for m in masks]
