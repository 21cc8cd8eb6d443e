"""From "a pattern on a text field" to "mask ready", in one process on one card: a byte automaton walked over the rows
(szg_mask_where_dfa) against the CONTAINS kernel that reads the same bytes, and against Python's `re` on the host.
The field holds synthetic addresses of 16 to 40 bytes, distinct per row; about one row in a hundred holds "needle".

  (a) col.contains(b"needle")            szg_mask_where_str, the existing kernel: the yardstick
  (b) col.dfa(compile("needle"))         the same question as an automaton: 7 states, in LDS
  (c) col.dfa(compile(EMAIL))            ^[^@\\s]+@[^@\\s]+\\.[a-z]{2,6}$: 84 states x 26 classes, in LDS
  (d) col.dfa(literal_set(500 stored))   a trie of about ten thousand states: walked in global memory
  (e) re.search over the same values     the host, what a Filter callable would do (3 repeats)

    python scripts/dev_where_dfa.py [--rows 1000000] [--repeats 20] [--out profiles/columns_where_dfa.txt]

Legs (a) to (d) alternate call by call in the same run; the automata are compiled before the clock starts (their
build times are reported apart), so each timing is what a cached pattern costs: the host's check and staging of the
table, the upload, the kernel, the download of the words.  Each timing is a host clock around a call that ends in a
device synchronise; every leg is warmed up first, the median of the repeats is reported with their spread, and every
count is checked against the host's.  The vectors are dim 8, 8-bit: the kernel does not read them.  One JSON line per
measurement.
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from syzgydb_amd import ScanIndex, regex_dfa  # noqa: E402

EMAIL = r"^[^@\s]+@[^@\s]+\.[a-z]{2,6}$"
EMAIL_PY = r"^[^@\t\n\f\r ]+@[^@\t\n\f\r ]+\.[a-z]{2,6}\Z"


def spread(samples):
    return {"median_ms": statistics.median(samples) * 1e3, "min_ms": min(samples) * 1e3, "max_ms": max(samples) * 1e3,
            "repeats": len(samples)}


def address(i):
    """16 to 40 bytes; one in a hundred holds "needle", one in seven is no address"""
    user = "u%07d" % ((i * 2654435761) % 10000000)
    if i % 100 == 37:
        user += ".needle"
    host = ("exa%d" % (i % 97)) + ("-m" * (i % 6))
    tld = ("com", "org", "info", "museum", "toolongt", "Org", "c1")[i % 7]
    return ("%s@%s.%s" % (user, host, tld)).encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.rows
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    values = [address(i) for i in range(n)]
    lengths = [len(v) for v in values]
    emit(path="values", rows=n, heap_bytes=sum(lengths), min_len=min(lengths), max_len=max(lengths))
    t0 = time.perf_counter()
    needle = regex_dfa.compile("needle")
    t1 = time.perf_counter()
    email = regex_dfa.compile(EMAIL)
    t2 = time.perf_counter()
    listed = values[::max(n // 500, 1)][:500]
    trie = regex_dfa.literal_set(listed)
    t3 = time.perf_counter()
    for name, d, dt in (("needle", needle, t1 - t0), ("email", email, t2 - t1), ("literal_set", trie, t3 - t2)):
        emit(path="compile", automaton=name, states=d.n_states, classes=d.n_classes, entries=d.entries, host_ms=dt * 1e3)
    inside = set(listed)
    want = {"a": sum(b"needle" in v for v in values), "d": sum(v in inside for v in values)}
    want["b"] = want["a"]
    # (e) the host: Python's re over the decoded values, as a Filter callable would walk them
    texts = [v.decode() for v in values]
    for name, pattern in (("needle", "needle"), ("email", EMAIL_PY)):
        rx = re.compile(pattern, re.ASCII)
        te = []
        for _ in range(3):
            t0 = time.perf_counter()
            count = sum(rx.search(t) is not None for t in texts)
            te.append(time.perf_counter() - t0)
        if name == "needle":
            assert count == want["a"]
        else:
            want["c"] = count
        emit(path="e: Python re.search over the values on the host", pattern=name, rows=n, count=count, **spread(te))
    with ScanIndex(8, 8, 1, devices=[0]) as ix:
        ix.synth(n, 7)
        col = ix.text_column(values)
        legs = [("a", "a: szg_mask_where_str CONTAINS \"needle\"", lambda: col.contains(b"needle")),
                ("b", "b: szg_mask_where_dfa, needle (LDS tier)", lambda: col.dfa(needle)),
                ("c", "c: szg_mask_where_dfa, email pattern (LDS tier)", lambda: col.dfa(email)),
                ("d", "d: szg_mask_where_dfa, literal_set of 500 (global tier)", lambda: col.dfa(trie))]
        for _ in range(2):   # warm-up, every leg
            for _, _, call in legs:
                call().close()
        times = {key: [] for key, _, _ in legs}
        for _ in range(args.repeats):
            for key, _, call in legs:
                t0 = time.perf_counter()
                m = call()
                times[key].append(time.perf_counter() - t0)
                assert m.count == want[key], (key, m.count, want[key])
                m.close()
        for key, name, _ in legs:
            emit(path=name, rows=n, count=want[key], **spread(times[key]))
        med = {key: statistics.median(times[key]) for key in times}
        emit(path="ratios of medians", b_over_a=med["b"] / med["a"], c_over_a=med["c"] / med["a"], d_over_b=med["d"] / med["b"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
