"""Who owns device memory (syzgydb_amd/csrc/dev_mem.h), on the card: every device block of a handle, a column or a
mask comes from one function that counts it and can be told to refuse the nth allocation on the host (no device fault:
hipMalloc is not called).  A refused compaction, reorder, column append or index append leaves everything as it was and
succeeds when repeated; and every lifetime gives back every block and byte it took."""
import gc

import numpy as np
import pytest

import oracle as orc
import test_gpu_column_carry as tcc
import test_gpu_text_columns as tgt
from syzgydb_amd import ScanIndex, SzgError, SZG_COSINE, _lib, reorder_plan
from syzgydb_amd.index import device_memory, refuse_device_alloc

pytestmark = pytest.mark.gpu

SEED, DIM, BITS = tcc.SEED, tcc.DIM, tcc.BITS
loaded_index, bits_equal = tcc.loaded_index, tcc.bits_equal
N = 300
ATTEMPTS = 200   # a cap, not a tuning number: the carry makes a few dozen allocations at this size


def memory_now():
    gc.collect()   # (handles an earlier test dropped without closing give their blocks back here, not in between)
    return device_memory()


def refused(call, nth):
    """call() with the nth device allocation refused: True when it was refused (SZG_E_NOMEM from the test hook), False
    when the call made fewer allocations and succeeded."""
    try:
        with refuse_device_alloc(nth):
            call()
    except SzgError as e:
        assert e.code == _lib.SZG_E_NOMEM and "refused: test hook" in str(e), e
        return True
    return False


def carried_index(devices, text, keep_bool, v):
    """300 rows with row 7 tombstoned; a mask, a text column with half its rows absent and an f64 column to carry."""
    ix = loaded_index(N, devices)
    if devices:
        ix.set_option("carry_stage_bytes", 4096)   # two shards: the staging windows repeat
    good, mask, unchanged = tcc.watch_index(ix, 7, N, text, keep_bool)
    f = ix.column(v)
    return ix, good, mask, f, unchanged


@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("how", ["compact", "reorder"])
def test_compact_and_reorder_under_refusals(how, devices):
    before = memory_now()
    text = tgt.values(N, np.random.default_rng(3))
    keep_bool = np.arange(N) % 5 != 0
    v = tcc.f64_values(N, 4)
    src = np.array([r for r in range(N) if r != 7][::-1])   # (reorder: every live row, reversed)
    ix, good, mask, f, unchanged = carried_index(devices, text, keep_bool, v)
    twin, t_good, t_mask, t_f, _ = carried_index(devices, text, keep_bool, v)

    def call(index, carry):
        if how == "compact":
            index.compact(carry=carry)
        else:
            index.reorder(src, carry=carry)

    call(twin, [t_mask, t_good, t_f])   # the unrefused run
    f_before = f.read()
    refusals = 0
    for nth in range(1, ATTEMPTS + 1):
        if not refused(lambda: call(ix, [mask, good, f]), nth):
            break
        refusals += 1
        unchanged()
        got = f.read()
        assert bits_equal(got[0], f_before[0]) and (got[1] == f_before[1]).all() and f.rows == N
        check = f.present()   # (still valid)
        check.close()
    else:
        pytest.fail("still refused after %d attempts" % ATTEMPTS)
    print("%s, devices=%s: %d refusals before the call went through" % (how, devices, refusals))
    assert refusals >= 1
    # what the refused-then-repeated handle holds is what the unrefused twin holds
    assert ix.rows == twin.rows == N - 1 and ix.live_rows == twin.live_rows
    assert (ix.read_rows(0, ix.rows) == twin.read_rows(0, twin.rows)).all()
    a, b = good.read(), t_good.read()
    assert a[0] == b[0] and (a[1] == b[1]).all() and good.info() == t_good.info()
    a, b = f.read(), t_f.read()
    assert bits_equal(a[0], b[0]) and (a[1] == b[1]).all() and f.info() == t_f.info()
    assert (mask.read() == t_mask.read()).all() and mask.count == t_mask.count
    m1, m2 = good.present(base=mask), t_good.present(base=t_mask)   # a where through the column and the mask
    assert (m1.read() == m2.read()).all() and m1.count == m2.count
    ix.close()
    twin.close()
    assert memory_now() == before


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_column_growth_under_refusals(devices):
    """A 1 000-row column on 2 200 rows: the append of the other 1 200 outgrows the capacity of the part that takes them
    (1 024 rows) on one shard and on two."""
    before = memory_now()
    total, have = 2200, 1000
    v = tcc.f64_values(total, 5)
    absent = np.arange(total) % 3 != 0
    text = [t if there else b"" for t, there in zip(tgt.values(total, np.random.default_rng(6)), absent)]   # (a row
    # that is absent when it arrives stores no bytes)
    with loaded_index(total, devices) as ix:
        f = ix.column(v[:have], present=absent[:have])
        t = ix.text_column(text[:have], present=absent[:have])
        for col, data, same in ((f, v, lambda x, y: bits_equal(x, y)), (t, text, lambda x, y: x == list(y))):
            was, info = col.read(), col.info()
            for nth in (1, 2):
                assert refused(lambda: col.append(data[have:], present=absent[have:]), nth)
                got = col.read()
                assert col.rows == have and same(got[0], was[0]) and (got[1] == was[1]).all()
                # (not the whole info(): on two shards the first part may have grown before the second was refused,
                # which moves device_bytes and reads the same)
                assert col.info()["rows"] == info["rows"] and col.info()["heap_used"] == info["heap_used"]
            col.append(data[have:], present=absent[have:])
            got = col.read()
            assert col.rows == total and same(got[0], data) and (got[1] == absent).all()
            tcc.check_mask(col.present(), absent)
    assert memory_now() == before


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_index_growth_under_refusals(devices):
    before = memory_now()
    rows = orc.synth_rows(SEED, 0, N + 100, DIM, BITS)
    with loaded_index(N, devices) as ix:
        was = ix.read_rows(0, N).copy()
        assert refused(lambda: ix.append(rows[N:]), 1)   # (the capacity after a load is the rows rounded up to 64)
        assert ix.rows == N and ix.live_rows == N and (ix.read_rows(0, N) == was).all()
        ix.append(rows[N:])
        assert ix.rows == N + 100 and (ix.read_rows(0, N + 100) == rows.reshape(N + 100, -1)).all()
    assert memory_now() == before


def sketched_index(devices, rows, queries, norms):
    """A float32 handle whose batch of 8 went through the 8-bit sketch pre-pass; norms=False: its grouped sweeps sum
    the rows' norms themselves (option scan_norms = 1, replayed on the sketch index), so no norm array is made."""
    ix = ScanIndex(DIM, 32, SZG_COSINE, devices=devices)
    ix.set_option("sketch", 1)        # (auto mode keeps no sketch for so few rows)
    ix.set_option("multi_query", 0)   # (a batch would share one sweep of the float32 rows instead of the pre-pass)
    if not norms:
        ix.set_option("scan_norms", 1)
    ix.load(rows)
    ix.search_topk(queries, 10)
    st = ix.stats()
    assert st["sketch_queries"] + st["sketch_fallbacks"] == 8   # the sketch index exists
    return ix


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_a_plain_lifetime_gives_everything_back(devices):
    before = memory_now()
    n = 5000
    rows = orc.synth_rows(SEED, 0, n, DIM, 32)
    queries = orc.synth_vectors(2, 0, 8, DIM)
    # the same handle without resident row norms: what it holds less is the norm arrays of the sketch shards, one
    # block of 4 bytes per row of capacity (the rows rounded up to 64) each
    plain = sketched_index(devices, rows, queries, norms=False)
    without = device_memory()
    plain.close()
    assert memory_now() == before
    ix = sketched_index(devices, rows, queries, norms=True)
    held = device_memory()
    counts = reorder_plan(n, np.arange(n), len(devices)) if devices else [n]
    print("devices=%s: held %s, without norms %s, shards %s" % (devices, held, without, counts))
    assert held[0] - without[0] == len(counts)
    assert held[1] - without[1] == sum(4 * ((c + 63) // 64 * 64) for c in counts)
    assert held[1] >= before[1] + rows.size
    col = ix.column(np.arange(n, dtype=np.float64))
    text = ix.text_column([b"row %d" % i for i in range(n)])
    mask = ix.mask(np.arange(n) % 2 == 0)
    for r in range(0, n, 7):
        ix.tombstone(r)
    ix.compact(carry=[col, text, mask])
    assert col.rows == ix.rows == n - len(range(0, n, 7))
    ix.search_topk(queries, 10)   # (a sketch for the new rows)
    ix.close()
    assert memory_now() == before
