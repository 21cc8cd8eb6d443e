"""What szg_set_option does with every option, written out by hand from the two if-chains the setter was before the
option table (csrc/options.cpp) replaced them: per name the default, whether szg_debug_option_check knows it, whether
the internal sketch index follows it, edge values that are accepted with what they store, edge values that are refused,
and the refusal's text.  tests/cpp/test_options.cpp carries the same list in C++; test_options_cpu.py holds the two
equal.  ("contexts" is the one option held against the handle: N_CTX contexts exist per shard.)"""

N_CTX = 4
MIB64 = 64 << 20


def _case(default, accepted, refused, text, check=False, forwarded=True, ok=None):
    return {"default": default, "accepted": accepted, "refused": refused, "text": text, "check": check,
            "forwarded": forwarded, "ok": ok}


def _same(*values):
    return [(v, v) for v in values]


BOOL = [(7, 1), (-1, 1), (0, 0), (1, 1)]   # every value is accepted; value != 0 is stored

CASES = {
    # not forwarded: the sketch index keeps its defaults
    "sketch": _case(2, _same(0, 1, 2), [-1, 3], "sketch is 0, 1 or 2", forwarded=False),
    "force_sketch_nomem": _case(0, BOOL, [], None, forwarded=False),
    "carry_stage_bytes": _case(0, _same(16, MIB64, 0), [8, -16, MIB64 + 16],
                               "carry_stage_bytes is 0 or a multiple of 16 up to 64 MiB", forwarded=False),
    "sketch_min_rows": _case(4096, [(1, 1), (1 << 40, 1 << 30), (1 << 30, 1 << 30), (5000, 5000)], [0, -1],
                             "sketch_min_rows out of range", forwarded=False),
    "sketch_list": _case(0, _same(4096, 0), [-1, 4097], "sketch_list out of range", forwarded=False),
    "sketch_extra": _case(30, _same(0, 900), [-1, 901], "sketch_extra out of range", forwarded=False),
    # forwarded
    "slack": _case(16, _same(0, 4096), [-1, 4097], "slack out of range"),
    "queries_per_launch": _case(16, _same(1, 16), [0, 17], "queries_per_launch out of range"),
    "scan_group": _case(0, _same(1, 2, 4, 0), [-1, 3, 5], "scan_group is 0, 1, 2 or 4", check=True, ok={0, 1, 2, 4}),
    "scan_group_ring": _case(0, _same(4, 6, 0), [-1, 1, 5, 7, 12], "scan_group_ring is 0 or a ring depth the library carries",
                             check=True, ok={0, 4, 6}),
    "scan_norms": _case(0, _same(1, 0), [-1, 2], "scan_norms is 0 or 1", check=True, ok={0, 1}),
    "sketch_planes": _case(0, _same(2, 3, 0), [-1, 1, 4], "sketch_planes is 0, 2 or 3", check=True, ok={0, 2, 3}),
    "sketch_matrix": _case(0, _same(1, 2, 0), [-1, 3], "sketch_matrix is 0, 1 or 2", check=True, ok={0, 1, 2}),
    "sketch_select": _case(0, _same(1, 0), [-1, 2], "sketch_select is 0 or 1", check=True, ok={0, 1}),
    "sketch_wide": _case(0, _same(1, 2, 0), [-1, 3], "sketch_wide is 0, 1 or 2", check=True, ok={0, 1, 2}),
    "sketch_share": _case(0, _same(1, 2, 0), [-1, 3], "sketch_share is 0, 1 or 2", check=True, ok={0, 1, 2}),
    "sketch_bulk": _case(0, _same(1024, 0), [-1, 1025], "sketch_bulk is 0 to 1024", check=True, ok=set(range(0, 1025))),
    "sketch_radius": _case(0, _same(1, 0), [-1, 2], "sketch_radius is 0 or 1", check=True, ok={0, 1}),
    "sketch_masked": _case(0, _same(1, 0), [-1, 2], "sketch_masked is 0 or 1", check=True, ok={0, 1}),
    "sketch_f64": _case(0, _same(1, 0), [-1, 2], "sketch_f64 is 0 or 1", check=True, ok={0, 1}),
    "sketch_topk_collect": _case(0, _same(1, 0), [-1, 2], "sketch_topk_collect is 0 or 1", check=True, ok={0, 1}),
    "query_prep": _case(0, _same(1, 2, 0), [-1, 3], "query_prep is 0, 1 or 2", check=True, ok={0, 1, 2}),
    "query_batch": _case(16, _same(1, 96), [0, 97], "query_batch out of range"),
    "radius_mq": _case(1, _same(0, 1), [-1, 2], "radius_mq is 0 or 1"),
    "finish_thread": _case(1, _same(0, 1), [-1, 2], "finish_thread is 0 or 1"),
    "contexts": _case(N_CTX, _same(1, N_CTX), [0, N_CTX + 1], "contexts out of range"),
    "multi_query": _case(1, BOOL, [], None),
    "mask_dense": _case(1, BOOL, [], None),
    "coalesce": _case(1, BOOL, [], None),
    "force_matrix": _case(0, BOOL, [], None),
    "force_no_refine": _case(0, BOOL, [], None),
    "mq_hits": _case(1024, _same(64, 65536), [63, 65537], "mq_hits out of range"),
    "mq_min": _case(2, _same(1, 32), [0, 33], "mq_min out of range"),
    "serialize_scans": _case(1, BOOL, [], None),
    "tie_mode": _case(0, _same(1, 0), [2, -1], "tie_mode must be 0 or 1"),
    "force_escalate": _case(0, BOOL, [], None),
}

ONE_SWEEP = [n for n, c in CASES.items() if c["check"]]           # what szg_debug_option_check answers for
FORWARDED = [n for n, c in CASES.items() if c["forwarded"]]
NOT_FORWARDED = [n for n, c in CASES.items() if not c["forwarded"]]
assert len(CASES) == 36 and len(ONE_SWEEP) == 14 and len(FORWARDED) == 30 and len(NOT_FORWARDED) == 6


def listing():
    """The list as tests/cpp/test_options.cpp prints its own under --list, one line per name in sorted order."""
    lines = []
    for name in sorted(CASES):
        c = CASES[name]
        lines.append("%s default=%d check=%d forwarded=%d accepted=%s refused=%s text=%s" % (
            name, c["default"], c["check"], c["forwarded"], ",".join("%d:%d" % p for p in c["accepted"]),
            ",".join("%d" % v for v in c["refused"]), c["text"] or ""))
    return lines
