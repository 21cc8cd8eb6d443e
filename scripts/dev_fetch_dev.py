"""Stored vectors out to device memory, and queries from it, against the only routes there were, in one process on one card:

  fetch   a   ScanIndex.fetch_into(t[, rows])                   (szg_index_fetch_rows_dev: decoded where the rows lie)
          b   read_rows + codec.decode_rows + torch.from_numpy(...).to(device)      (packed bytes to the host, decoded
                                                                 there, cast to the tensor's type, uploaded again)
          for 32-bit rows -> float32, 8-bit rows -> bfloat16, and 64-bit rows -> float32 with a list of 100 000 random rows
          (route b reads the whole range, picks the listed rows on the host and decodes those)
  query   a   ScanIndex.search_topk_tensor(t, 10)               (szg_search_topk_dev: converted on the card, one copy down)
          b   ScanIndex.search_topk(t.cpu().double().numpy(), 10)
          for 1 024 float32 queries on a float32 handle under the default options

    python scripts/dev_fetch_dev.py [--rows 1000000] [--dim 768] [--repeats 5] [--out profiles/fetch_dev.txt]

Each timing of a leg is a host clock around the WHOLE cost to the caller, ending with the values on the card (a
synchronises inside; b ends in a device synchronise).  The legs alternate call by call, one warm-up call per leg, then the
median of the repeats with their spread; after each pair the two results are compared on their bits.
The fetch kernel's own time is taken by device events around fetch_into of the whole 32-bit handle into a float32 tensor
that exists already: nothing is allocated in the window, what remains beside the kernel is its launch.  Its rate is the bytes
it must move -- n x row_bytes read plus n x dim x 4 written -- over that time.  The yardstick is taken in the same job: the
ingest encoder the other way (events around append_tensor of a float32 tensor into a 32-bit handle whose capacity has been
reserved, as scripts/dev_ingest_dev.py takes it: the same bytes moved), and a device-to-device copy of the same tensor
(events around Tensor.copy_, 2 x n x dim x 4 bytes).  One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from syzgydb_amd import ScanIndex, SZG_COSINE, codec  # noqa: E402

INTS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def spread(samples):
    return {"median_ms": statistics.median(samples) * 1e3, "min_ms": min(samples) * 1e3, "max_ms": max(samples) * 1e3,
            "repeats": len(samples)}


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def filled(bits, n, dim, src_dtype):
    """A handle of n rows appended from a random tensor on the card (the tensor is dropped)."""
    ix = ScanIndex(dim, bits, SZG_COSINE, devices=[0])
    t = (torch.rand((n, dim), device="cuda:0", dtype=torch.float32) * 2.5 - 1.25).to(src_dtype)
    ix.append_tensor(t)
    del t
    return ix


def fetch_case(name, bits, dtype, n, dim, repeats, emit, listed=0):
    ix = filled(bits, n, dim, torch.float64 if bits == 64 else torch.float32)
    rows = np.random.default_rng(5).integers(0, n, size=listed) if listed else None
    m = listed or n
    out = torch.empty((m, dim), dtype=dtype, device="cuda:0")
    ta, tb = [], []
    try:
        for i in range(repeats + 1):   # call 0 warms both legs up
            out.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix.fetch_into(out, rows=rows)
            t1 = time.perf_counter()
            data = ix.read_rows(0, n)
            if rows is not None:
                data = data[rows]
            host = torch.from_numpy(codec.decode_rows(data, dim, bits)).float()
            up = (host if dtype == torch.float32 else host.to(dtype)).to("cuda:0")
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            equal = bool(torch.equal(out.view(INTS[dtype]), up.view(INTS[dtype])))
            assert equal
            del data, host, up
            if i:
                ta.append(t1 - t0)
                tb.append(t2 - t1)
            emit(path=name + " call", call=i, fetch_ms=(t1 - t0) * 1e3, host_ms=(t2 - t1) * 1e3, values_equal=equal)
        emit(path=name + " a: fetch_into", rows=m, of_rows=n, dim=dim, bits=bits, dest=str(dtype), **spread(ta))
        emit(path=name + " b: read_rows + decode_rows + from_numpy().to(device)", rows=m, of_rows=n, dim=dim, bits=bits,
             dest=str(dtype), **spread(tb), ratio_b_over_a=statistics.median(tb) / statistics.median(ta), values_equal=True)
    finally:
        ix.close()


def kernel_case(n, dim, repeats, emit):
    """The fetch kernel, the ingest encoder and a device-to-device copy, each moving n x dim x 8 bytes, by events."""
    src = torch.rand((n, dim), device="cuda:0", dtype=torch.float32) * 2.5 - 1.25
    out = torch.empty_like(src)
    tf, te, tc = [], [], []
    with ScanIndex(dim, 32, SZG_COSINE, devices=[0]) as ix, ScanIndex(dim, 32, SZG_COSINE, devices=[0]) as c:
        ix.append_tensor(src)
        row_bytes = ix.row_bytes
        for i in range(repeats + 1):   # call 0 warms every leg up
            fetch = events(lambda: ix.fetch_into(out))
            c.synth(n, 7)
            c.load(np.zeros((0, c.row_bytes), dtype=np.uint8))   # no rows, the capacity stays
            enc = events(lambda: c.append_tensor(src))
            assert c.rows == n
            copy = events(lambda: out.copy_(src))
            if i:
                tf.append(fetch), te.append(enc), tc.append(copy)
            emit(path="kernels call", call=i, fetch_ms=fetch * 1e3, encoder_ms=enc * 1e3, copy_ms=copy * 1e3)
        ix.fetch_into(out)
        equal = bool(torch.equal(out, src))   # (32-bit rows hold the float32 values themselves)
        assert equal
    moved = n * (row_bytes + dim * 4)
    fetch_rate, enc_rate, copy_rate = (moved / statistics.median(t) for t in (tf, te, tc))
    emit(path="float32 -> 32-bit encoder (events, capacity reserved)", bytes_moved=moved, **spread(te), bytes_per_s=enc_rate)
    emit(path="device-to-device copy (events, Tensor.copy_)", bytes_moved=moved, **spread(tc), bytes_per_s=copy_rate)
    emit(path="32-bit -> float32 fetch kernel (events, contiguous)", bytes_moved=moved, **spread(tf), bytes_per_s=fetch_rate,
         share_of_encoder_rate=fetch_rate / enc_rate, share_of_copy_rate=fetch_rate / copy_rate, values_equal=equal)


def query_case(n, dim, nq, k, repeats, emit):
    ta, tb = [], []
    with ScanIndex(dim, 32, SZG_COSINE, devices=[0]) as ix:
        ix.synth(n, 7)
        t = torch.rand((nq, dim), device="cuda:0", dtype=torch.float32) * 1.6 - 0.8
        torch.cuda.synchronize()
        for i in range(repeats + 1):   # call 0 warms both legs up (and builds what the default options keep beside the rows)
            t0 = time.perf_counter()
            got = ix.search_topk_tensor(t, k)
            t1 = time.perf_counter()
            want = ix.search_topk(t.cpu().double().numpy(), k)
            t2 = time.perf_counter()
            equal = bool((got[0] == want[0]).all() and (got[1].view(np.uint64) == want[1].view(np.uint64)).all()
                         and (got[2] == want[2]).all())
            assert equal
            if i:
                ta.append(t1 - t0)
                tb.append(t2 - t1)
            emit(path="queries call", call=i, tensor_ms=(t1 - t0) * 1e3, host_ms=(t2 - t1) * 1e3, answers_equal=equal)
    emit(path="queries a: search_topk_tensor", rows=n, dim=dim, queries=nq, k=k, **spread(ta))
    emit(path="queries b: cpu().double().numpy() + search_topk", rows=n, dim=dim, queries=nq, k=k, **spread(tb),
         ratio_b_over_a=statistics.median(tb) / statistics.median(ta), answers_equal=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--listed", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)
        if args.out:   # (written as it goes: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")

    emit(path="setup", rows=args.rows, dim=args.dim, repeats=args.repeats, device=torch.cuda.get_device_name(0))
    kernel_case(args.rows, args.dim, args.repeats, emit)
    query_case(args.rows, args.dim, args.queries, 10, args.repeats, emit)
    fetch_case("32-bit -> float32", 32, torch.float32, args.rows, args.dim, args.repeats, emit)
    fetch_case("8-bit -> bfloat16", 8, torch.bfloat16, args.rows, args.dim, args.repeats, emit)
    fetch_case("64-bit -> float32, %d listed rows" % min(args.listed, args.rows), 64, torch.float32, args.rows, args.dim,
               args.repeats, emit, listed=min(args.listed, args.rows))


if __name__ == "__main__":
    main()
