"""Ingest from device memory against the only route there was from the same tensor, in one process on one card:

  a   ScanIndex.append_tensor(t)                             (szg_index_append_dev: the encoder reads the tensor in place)
  b   ScanIndex.append_vectors(t.cpu().double().numpy())     (the tensor to the host, widened to float64 there, and the
                                                             float64 data back through the staging block in 64 MiB chunks)

for two cases at 1M x 768: a float32 tensor into a 32-bit handle and a bfloat16 tensor into an 8-bit handle.

    python scripts/dev_ingest_dev.py [--rows 1000000] [--dim 768] [--repeats 5] [--out profiles/ingest_dev.txt]

Each timing is a host clock around the WHOLE cost to the caller -- for b that includes the copy down and the widening --
and both calls return with the rows resident (they synchronise inside).  Every call gets a fresh handle, so each pays for
its rows' block; the legs alternate call by call, one warm-up call per leg, then the median of the repeats with their
spread.  After each pair the two handles' rows are read back at 64 positions and compared.
The encoder's own time is taken by device events around append_tensor on a third handle whose capacity has been reserved
beforehand (a synth of as many rows, then an empty load): nothing is allocated inside the window, what remains beside the
kernel is its launch and the copy of the new live words (n / 8 bytes).  Its rate is the bytes it must move -- n x dim x
source bytes read plus n x row_bytes written -- over that time, set beside the card's measured copy rate (6.29 TB/s, a
float4 copy), not the spec peak.  One JSON line per measurement.
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

from syzgydb_amd import ScanIndex, SZG_COSINE  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s, measured float4 copy on this card


def spread(samples):
    return {"median_ms": statistics.median(samples) * 1e3, "min_ms": min(samples) * 1e3, "max_ms": max(samples) * 1e3,
            "repeats": len(samples)}


def run_case(name, dtype, bits, n, dim, repeats, emit):
    t = (torch.rand((n, dim), device="cuda:0", dtype=torch.float32) * 2.5 - 1.25).to(dtype)
    torch.cuda.synchronize()
    probe = np.unique(np.linspace(0, n - 1, 64).astype(np.int64))
    ta, tb, te = [], [], []
    row_bytes = 0
    for i in range(repeats + 1):   # call 0 warms both legs up
        with ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as a, ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as b:
            row_bytes = a.row_bytes
            t0 = time.perf_counter()
            a.append_tensor(t)
            t1 = time.perf_counter()
            b.append_vectors(t.cpu().double().numpy())
            t2 = time.perf_counter()
            assert a.rows == b.rows == n
            equal = all((a.read_rows(int(r), 1) == b.read_rows(int(r), 1)).all() for r in probe)
            assert equal
        with ScanIndex(dim, bits, SZG_COSINE, devices=[0]) as c:
            c.synth(n, 7)
            c.load(np.zeros((0, c.row_bytes), dtype=np.uint8))   # no rows, the capacity stays
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            c.append_tensor(t)
            e1.record()
            e1.synchronize()
            enc = e0.elapsed_time(e1) * 1e-3
            assert c.rows == n
        if i:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
            te.append(enc)
        emit(path=name + " call", call=i, tensor_ms=(t1 - t0) * 1e3, host_ms=(t2 - t1) * 1e3, encoder_ms=enc * 1e3, rows_equal=equal)
    moved = n * dim * t.element_size() + n * row_bytes
    emit(path=name + " a: append_tensor", rows=n, dim=dim, bits=bits, source=str(dtype), **spread(ta))
    emit(path=name + " b: cpu().double().numpy() + append_vectors", rows=n, dim=dim, bits=bits, source=str(dtype), **spread(tb),
         ratio_b_over_a=statistics.median(tb) / statistics.median(ta))
    rate = moved / statistics.median(te)
    emit(path=name + " encoder (events, capacity reserved)", bytes_moved=moved, **spread(te), bytes_per_s=rate,
         measured_copy_rate=COPY_RATE, share_of_copy_rate=rate / COPY_RATE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    emit(path="setup", rows=args.rows, dim=args.dim, repeats=args.repeats, device=torch.cuda.get_device_name(0))
    run_case("float32 -> 32-bit", torch.float32, 32, args.rows, args.dim, args.repeats, emit)
    run_case("bfloat16 -> 8-bit", torch.bfloat16, 8, args.rows, args.dim, args.repeats, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
