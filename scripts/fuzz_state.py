"""Stateful, model-based fuzzing of ScanIndex: mutations, masks, columns, readers and searches on ONE handle per case.

    python scripts/fuzz_state.py SEED --cases N [--profile plain|sketched] [--plan-only] [--certificates]

Every case opens one handle (random width, metric, dimension, one or two shards, random options), loads it, and runs 8 to 25
operations drawn from every mutation, mask, column, reader and search entry point of the handle.  Beside the handle a MODEL
lives on the host -- the packed rows in the reference encoding, the live bits, the row base, every mask as a bool array with
its stale flag, one float64 and one text column -- and it never asks the library what the truth is: rows come from
oracle.encode_rows, answers from oracle.search_exact over the model's rows with allow = live & filter (same rows in the same
order, float64 distances equal on the bits, NaN == NaN), fetched tensors from the codec and the cast chain float64 ->
float32 -> float16 / bfloat16.  After every mutation rows, live_rows and read_rows(0, rows) must be the model's.

The case count is fixed and there is no time budget: a seed means the same cases on every run and every card.  Everything
the generator decides depends on the model alone and every case has a random stream of its own (seed, case number), so --plan-only (generator, model and oracle; no handle, no torch) prints
the plan the card would run.

Profiles: `plain` draws every width and the launch-shape options; `sketched` keeps to 32- and 64-bit rows in whole 64-byte
steps of the 8-bit sketch with sketch = 1 and draws the options that are soaking (sketch_masked, sketch_radius, sketch_f64,
sketch_topk_collect) beside the matrix sweep's forms.

A mismatch prints the case and its operation log (enough to replay it by hand), ends the case and counts as a failure; an
exception the model did not predict -- a device error, anything from torch -- ends the WHOLE run with exit status 2 and opens
no further handle.  Refusals the model predicts (a stale mask, a short column, a row listed twice, a row out of range) are
asserted by code and text.  The last line is one JSON object: cases, failures, operation counts, `plan` -- a digest of every
case's operation log, the same with and without a card as long as no case fails -- and `served`, the path counters summed
over the handles.  --certificates checks every search's certificate trace with cert_check, as fuzz_gpu.py --certificates does;
while the row base is not 0 the records are read and dropped, because the checker numbers rows from 0.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

DTYPES = ("f64", "f32", "f16", "bf16")
U64_MAX = 0xFFFFFFFFFFFFFFFF
TAG_NEAR = 0x6E656172
TAG_STATE = 0x73746174
NQS = [1, 2, 7, 16, 17, 33, 50, 70]
KS = [1, 10, 34, 35, 50, 100, 300]
DIMS = [1, 3, 33, 64, 100, 128, 192]
# fuzz_gpu.py's OPTS (tie_mode stays 0)
OPTS = [("queries_per_launch", [1, 3, 16]), ("multi_query", [0, 1]), ("force_matrix", [0, 0, 1]),
        ("serialize_scans", [0, 1]), ("mq_min", [2, 8]), ("slack", [0, 16, 40]), ("mq_hits", [64, 1024]),
        ("sketch", [0, 1, 1]), ("sketch_extra", [0, 30]), ("sketch_min_rows", [1, 1, 4096]),
        ("force_no_refine", [0, 0, 1]), ("mask_dense", [0, 1]), ("coalesce", [0, 1]), ("finish_thread", [0, 1, 1]),
        ("radius_mq", [0, 1, 1]), ("query_batch", [5, 16]), ("scan_group", [0, 1, 2, 4]), ("sketch_radius", [0, 1, 1]),
        ("sketch_share", [0, 1, 2, 2]), ("sketch_topk_collect", [0, 1, 1])]
PLAIN_MORE = [("scan_norms", [0, 1]), ("scan_group_ring", [0, 4, 6]), ("contexts", [1, 4])]
SKETCHED = [("sketch_masked", [0, 1]), ("sketch_radius", [0, 1]), ("sketch_topk_collect", [0, 1]), ("sketch_matrix", [0, 0, 1, 2, 2]),
            ("sketch_select", [0, 1]), ("sketch_wide", [0, 1, 2]), ("sketch_share", [0, 1, 2]), ("sketch_bulk", [0, 1, 2]),
            ("sketch_planes", [0, 0, 0, 3]), ("sketch_list", [0, 4, 64]), ("sketch_extra", [0, 30]), ("multi_query", [0, 0, 1]),
            ("radius_mq", [0, 0, 1])]
# options the header says invalidate nothing resident: drawn again once in the middle of a case
REDRAW = [("sketch_planes", [0, 3]), ("queries_per_launch", [1, 3, 16]), ("scan_group", [0, 1, 2, 4]),
          ("scan_group_ring", [0, 4, 6]), ("query_batch", [5, 16])]
FVALS = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -2.0, 3.0, 1e300, -1e-300])
CMP = {"==": np.equal, "!=": np.not_equal, "<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}
ALPHABET = (b"a", b"b", b"\x00", b"\xff")
SERVED = ("sketch_queries", "sketch_fallbacks", "sketch_radius_queries", "mq_queries", "mq_bf16_sweeps", "escalations",
          "full_replays")

# (kind, weight): an operation that cannot apply is drawn again
WEIGHTS = [("append", 2), ("append_vectors", 2), ("append_tensor", 4),
           ("overwrite", 2), ("overwrite_vector", 2), ("overwrite_rows", 2), ("overwrite_vectors", 2), ("overwrite_tensor", 4),
           ("tombstone", 2), ("tombstone_rows", 3), ("tombstone_mask", 2), ("compact", 4), ("reorder", 3),
           ("mask_bool", 2), ("mask_words", 2), ("mask_rows", 2), ("mask_and", 2), ("mask_or", 2), ("mask_not", 2),
           ("mask_andnot", 2), ("mask_count", 2), ("mask_read", 2),
           ("col_new", 4), ("col_append", 4), ("col_set_rows", 3), ("col_set", 3), ("where", 12), ("isin", 3), ("present", 3),
           ("startswith", 3), ("contains", 3), ("text_eq", 3),
           ("search_topk", 8), ("search_radius", 4), ("search_radius_capacity", 3), ("search_radius_batch", 4),
           ("search_topk_tensor", 6), ("search_radius_tensor", 5),
           ("fetch_range", 4), ("fetch_list", 4), ("distances", 2), ("pair_distances", 2), ("set_row_base", 2),
           ("refuse_stale_mask", 6), ("refuse_short_column", 5), ("refuse_twice", 2), ("refuse_range", 2)]
KINDS = [k for k, _ in WEIGHTS]


# ---- the comparisons: plain numpy, no device ---------------------------------------------------------------------------
def pack_bits(a):
    """bool[n] -> uint64 words, bit r of word r // 64, tail bits 0."""
    a = np.asarray(a, dtype=bool).reshape(-1)
    padded = np.zeros((a.size + 63) // 64 * 64, dtype=np.uint8)
    padded[:a.size] = a
    return np.packbits(padded, bitorder="little").view(np.uint64)


def same_answer(got_rows, got_dist, want_rows, want_dist, live=None, base=0):
    """The oracle's answer: the same rows in the same order, float64 distances equal on the bits (NaN == NaN); with
    `live`, no hit may be a tombstoned row whatever the yardstick says."""
    gr = np.asarray(got_rows, dtype=np.uint64).reshape(-1)
    wr = np.asarray(want_rows, dtype=np.uint64).reshape(-1)
    g = np.ascontiguousarray(got_dist, dtype=np.float64).reshape(-1)
    w = np.ascontiguousarray(want_dist, dtype=np.float64).reshape(-1)
    if gr.size != wr.size or g.size != w.size or g.size != gr.size or not (gr == wr).all():
        return False
    if live is not None and gr.size:
        live = np.asarray(live, dtype=bool)
        local = gr.astype(np.int64) - int(base)
        if (local < 0).any() or (local >= live.size).any() or not live[local].all():
            return False
    return bool(((g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))).all())


def same_rows(got, want):
    """Packed rows, byte for byte."""
    got, want = np.asarray(got, dtype=np.uint8), np.asarray(want, dtype=np.uint8)
    return got.shape == want.shape and bool((got == want).all())


def same_mask(got_words, want):
    """A mask's words against bool[rows]: every bit, the tail word's zero bits included."""
    got = np.asarray(got_words, dtype=np.uint64).reshape(-1)
    w = pack_bits(want)
    return got.size == w.size and bool((got == w).all())


def same_column(got_values, got_present, want_values, want_present):
    """A column as read() returns it against the model: the present bits of every row, and the values of the present rows
    on the bits (float64: NaN's and the sign of zero count) or as bytes (text)."""
    gp, wp = np.asarray(got_present, dtype=bool), np.asarray(want_present, dtype=bool)
    if gp.shape != wp.shape or not (gp == wp).all() or len(got_values) != len(want_values):
        return False
    if isinstance(want_values, np.ndarray):
        g = np.ascontiguousarray(got_values, dtype=np.float64).view(np.uint64)
        w = np.ascontiguousarray(want_values, dtype=np.float64).view(np.uint64)
        return bool((g[wp] == w[wp]).all())
    return all(bytes(a) == bytes(b) for a, b, p in zip(got_values, want_values, wp) if p)


def _bits_of(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:   # bfloat16 travels as its bits
        return a, (a & 0x7FFF) > 0x7F80
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16}[a.dtype.itemsize]), np.isnan(a)


def same_tensor_bits(got, want):
    """Two arrays of one float type (float64 / float32 / float16, or uint16 holding bfloat16) equal on the bits, NaNs equal:
    -0.0 is not +0.0."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    (g, gn), (w, wn) = _bits_of(got), _bits_of(want)
    return bool((gn == wn).all() and (g[~wn] == w[~wn]).all())


def round_to(v, name):
    """float64 values rounded (to nearest even) to the named type and widened back: exact in that type."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    if name == "f64":
        return v.copy()
    if name == "f16":
        return v.astype(np.float16).astype(np.float64)
    f = v.astype(np.float32)
    if name == "bf16":
        b = f.view(np.uint32).astype(np.uint64)
        f = (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return f.astype(np.float64)


class Mismatch(Exception):
    pass


# ---- the device side: torch is imported only when a card is used ----------------------------------------------------------
class Card:
    def __init__(self):
        import torch
        self.torch = torch
        self.types = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

    def tensor(self, v64, name):
        """Values exact in `name` (round_to) as a tensor of that type on card 0."""
        return self.torch.from_numpy(np.ascontiguousarray(v64, dtype=np.float64)).to(self.types[name]).cuda()

    def bits(self, t):
        t = t.detach().cpu().contiguous()
        if t.dtype == self.torch.bfloat16:
            return t.view(self.torch.int16).numpy().view(np.uint16)
        return t.numpy()

    def chain(self, f64, name):
        """The header's rule on the CPU: float64 -> (one cast) float32 -> (one more) float16 / bfloat16."""
        t = self.torch.from_numpy(np.array(f64, dtype=np.float64))
        if name != "f64":
            t = t.float()
            if name != "f32":
                t = t.to(self.types[name])
        return self.bits(t)


class Case:
    """One handle and its model."""

    def __init__(self, fz, no):
        self.fz, self.no, self.card = fz, no, fz.card
        # a stream per case: a case's plan depends on (seed, profile, case number) alone, whatever happened before it
        self.rng = np.random.default_rng([fz.args.seed, TAG_STATE, no])
        self.near = np.random.default_rng([fz.args.seed, TAG_NEAR, no])   # the near-row queries' own
        self.log, self.ix = [], None
        self.masks, self.fcol, self.tcol = [], None, None   # masks: dicts {id, arr, stale, h}; columns: {vals, pres, h}
        self.mask_no = 0

    # -- small helpers ------------------------------------------------------------------------------------------------------
    def choice(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def note(self, text):
        self.log.append(text)

    def count(self, key):
        self.fz.counts[key] = self.fz.counts.get(key, 0) + 1

    def fail(self, what):
        raise Mismatch(what)

    def refused(self, fn, code, text):
        from syzgydb_amd import SzgError, _lib
        try:
            fn()
        except SzgError as e:
            if e.code == _lib.SZG_E_DEVICE:
                raise
            if e.code != code or text not in str(e):
                self.fail("refusal %r: expected code %d and %r" % (str(e), code, text))
            return
        self.fail("not refused: expected code %d, %r" % (code, text))

    def encode(self, v):
        return self.fz.orc.encode_rows(np.atleast_2d(v), self.bits)

    def vectors(self, m):
        return self.rng.uniform(-1, 1, (m, self.dim)) * float(self.choice([1.0, 1.0, 0.3]))

    def split(self, n):
        per = (-(-n // self.n_shards) + 63) & ~63
        out, left = [], n
        for _ in range(self.n_shards):
            out.append(min(per, left))
            left -= out[-1]
        return out

    def current(self):
        return [m for m in self.masks if not m["stale"]]

    def check_state(self):
        if self.ix is None:
            return
        n = len(self.rows)
        if self.ix.rows != n or self.ix.live_rows != int(self.live.sum()):
            self.fail("rows %d live %d, model %d %d" % (self.ix.rows, self.ix.live_rows, n, int(self.live.sum())))
        got = self.ix.read_rows(0, n)
        if not same_rows(got, self.rows):
            self.fail("read_rows differs from the model at rows %s" % np.argwhere((got != self.rows).any(axis=1))[:8].ravel())

    # -- the case -----------------------------------------------------------------------------------------------------------
    def draw(self):
        rng, fz = self.rng, self.fz
        sk = fz.profile == "sketched"
        self.bits = int(self.choice([32, 64] if sk else [4, 8, 16, 32, 64]))
        self.metric = int(rng.integers(0, 2))
        lattice = [c.dim for c in fz.lattice.cells(self.bits)]
        self.dim = int(self.choice([64, 128, 192] if sk else DIMS + [self.choice(lattice)]))
        self.n_shards = 2 if rng.random() < 0.3 else 1
        if sk:
            opts = {name: int(self.choice(vals)) for name, vals in SKETCHED}
            opts.update(sketch=1, sketch_min_rows=1)
            if self.bits == 64:
                opts["sketch_f64"] = 1
            n = int(self.choice([400, 700, 1000, 2000]) if rng.random() < 0.6 else self.choice([1, 17, 65, 200, 399]))
        else:
            opts = {name: int(self.choice(vals)) for name, vals in OPTS + PLAIN_MORE if rng.random() < 0.3}
            n = int(self.choice([1, 2, 17, 63, 64, 65, 200, 400, 1000, 3000]))
        self.opts = opts
        self.n0 = max(1, min(n, 400_000 // self.dim))
        self.base = 0
        self.desc = dict(case=self.no, profile=fz.profile, bits=self.bits, metric=self.metric, dim=self.dim,
                         shards=self.n_shards, rows=self.n0, opts=opts)
        self.count("bits:%d" % self.bits)
        self.count("shards:%d" % self.n_shards)
        for name in ("sketch_masked", "sketch_radius", "sketch_f64", "sketch_topk_collect"):
            if opts.get(name) == 1:
                self.count("option:%s" % name)

    def run(self):
        self.draw()
        self.note("CASE %s" % json.dumps(self.desc))
        if self.card is not None:
            from syzgydb_amd import ScanIndex
            self.ix = ScanIndex(self.dim, self.bits, self.metric, devices=[0] * self.n_shards)
        try:
            if self.ix is not None:
                for name, val in self.opts.items():
                    self.ix.set_option(name, val)
                if self.fz.args.certificates:
                    self.ix.trace_certificates(True)
            self.rows = np.zeros((0, self.fz.orc.vector_size(self.bits, self.dim)), dtype=np.uint8)
            self.live = np.zeros(0, dtype=bool)
            self.shards = [0] * self.n_shards
            self.op_append(self.choice(["load", "append_vectors", "append_tensor"]), self.n0)
            while self.rng.random() < 0.6 and self.apply("col_new"):   # most cases start with a column or two
                self.count("col_new")
            n_ops = int(self.rng.integers(8, 26))
            redraw_at = int(self.rng.integers(1, n_ops))
            w = np.array([x for _, x in WEIGHTS], dtype=np.float64)
            w /= w.sum()
            done = 0
            while done < n_ops:
                kind = KINDS[int(self.rng.choice(len(KINDS), p=w))]
                if self.apply(kind) is False:
                    continue
                self.count(kind)
                done += 1
                while kind.startswith("append") and self.rng.random() < 0.7 and self.apply("col_append"):
                    self.count("col_append")   # the columns are brought level with the rows, more often than not at once
                if done == redraw_at:
                    name, vals = self.choice(REDRAW)
                    val = int(self.choice(vals))
                    self.note("set_option %s = %d" % (name, val))
                    self.opts[name] = val
                    self.count("option_redraw")
                    if self.ix is not None:
                        self.ix.set_option(name, val)
        except Mismatch:
            self.finish()
            raise
        self.finish()   # (after any other exception the handle is left alone: no further call into the library)

    def finish(self):
        if self.ix is not None:
            self.fz.collect(self.ix, self.bits)
            self.ix.close()
            self.ix = None

    def apply(self, kind):
        if kind in ("append", "append_vectors", "append_tensor"):
            return self.op_append(kind, int(self.choice([1, 2, 17, 40, 130, 300])))
        if kind.startswith("overwrite"):
            return self.op_overwrite(kind)
        if kind.startswith("tombstone"):
            return self.op_delete(kind)
        if kind in ("compact", "reorder"):
            return self.op_move(kind)
        if kind.startswith("mask_"):
            return self.op_mask(kind)
        if kind in ("col_new", "col_append", "col_set_rows", "col_set"):
            return self.op_column(kind)
        if kind in ("where", "isin", "present", "startswith", "contains", "text_eq"):
            return self.op_where(kind)
        if kind.startswith("search_"):
            return self.op_search(kind)
        if kind.startswith("fetch_"):
            return self.op_fetch(kind)
        if kind in ("distances", "pair_distances"):
            return self.op_distances(kind)
        if kind == "set_row_base":
            self.base = int(self.choice([0, 0, 1000, 1 << 40]))
            self.note("set_row_base %d" % self.base)
            if self.ix is not None:
                self.ix.set_row_base(self.base)
            return True
        return self.op_refusal(kind)

    # -- tensors of vectors ---------------------------------------------------------------------------------------------------
    def source(self, m, what):
        """m vectors that arrive as a tensor: (values exact in the drawn type, [m, dim]; a function that builds the tensor
        and the src_rows of the call on the card).  Draws the type, a column slice of a wider tensor, and a list of source
        rows with duplicates."""
        dt = self.choice(DTYPES)
        listed = self.rng.random() < 0.5
        p = int(self.rng.integers(max(1, m - 2), m + 3)) if listed else m
        pad = int(self.choice([0, 0, 5]))
        off = int(self.rng.integers(0, pad + 1))
        wide = round_to(self.rng.uniform(-1, 1, (p, self.dim + pad)) * float(self.choice([1.0, 1.0, 0.3])), dt)
        src = None
        if listed:   # any order, and a few rows twice (more would tie distances and send the sketch's calls to the full replay)
            src = self.rng.permutation(max(p, m))[:m] % p
            src[self.rng.integers(0, m, 2)] = src[self.rng.integers(0, m, 2)]
        vals = wide[:, off:off + self.dim][src if listed else slice(None)]
        self.count("%s:%s" % (what, dt))
        self.note("  tensor %s pool %d stride %d offset %d src_rows %s" % (dt, p, self.dim + pad, off,
                                                                         None if src is None else src.tolist()))

        def build():
            return self.card.tensor(wide, dt)[:, off:off + self.dim], src
        return vals, build

    # -- mutations ----------------------------------------------------------------------------------------------------------
    def op_append(self, kind, m):
        n = len(self.rows)
        m = min(m, 600_000 // self.dim - n, 4500 - n) if n else m
        if m < 1:
            return False
        self.note("%s %d rows (then %d)" % (kind, m, n + m))
        if kind == "append_tensor":
            v, build = self.source(m, kind)
        else:
            v = self.vectors(m)
        new = self.encode(v)
        if self.ix is not None:
            if kind == "load":
                self.ix.load(new)
            elif kind == "append":
                self.ix.append(new)
            elif kind == "append_vectors":
                self.ix.append_vectors(v)
            else:
                t, src = build()
                self.ix.append_tensor(t, src_rows=src)
        self.rows = np.concatenate([self.rows, new])
        self.live = np.concatenate([self.live, np.ones(m, dtype=bool)])
        if kind == "load":
            self.shards = self.split(m)
        else:
            self.shards[-1] += m
        for mk in self.masks:
            mk["stale"] = True
        self.check_state()
        return True

    def op_overwrite(self, kind):
        n = len(self.rows)
        single = kind in ("overwrite", "overwrite_vector")
        m = 1 if single else min(n, int(self.choice([1, 3, 20, 100])))
        at = self.rng.choice(n, size=m, replace=False).astype(np.uint64)
        self.note("%s rows %s" % (kind, at.tolist()))
        if kind == "overwrite_tensor":
            v, build = self.source(m, kind)
        else:
            v = self.vectors(m) * float(self.rng.random() >= 0.1)   # (now and then zero vectors)
        new = self.encode(v)
        if self.ix is not None:
            if kind == "overwrite":
                self.ix.overwrite(int(at[0]), new[0])
            elif kind == "overwrite_vector":
                self.ix.overwrite_vector(int(at[0]), v[0])
            elif kind == "overwrite_rows":
                self.ix.overwrite_rows(at, new)
            elif kind == "overwrite_vectors":
                self.ix.overwrite_vectors(at, v)
            else:
                t, src = build()
                self.ix.overwrite_tensor(at, t, src_rows=src)
        self.rows[at.astype(np.int64)] = new
        self.check_state()
        return True

    def op_delete(self, kind):
        n = len(self.rows)
        if kind == "tombstone":
            at = np.array([int(self.rng.integers(0, n))])
        elif kind == "tombstone_rows":   # duplicates and rows that are dead already
            at = self.rng.integers(0, n, min(2 * n, int(self.choice([1, 5, 40, 200]))))
        else:
            mk = self.a_mask(sparse=True)
            at = np.flatnonzero(mk["arr"])
        want = int(self.live[np.unique(at)].sum()) if at.size else 0
        self.note("%s %s -> %d dropped" % (kind, "mask %d" % mk["id"] if kind == "tombstone_mask" else at.tolist(), want))
        if self.ix is not None:
            if kind == "tombstone":
                self.ix.tombstone(int(at[0]))
            else:
                got = self.ix.tombstone_rows(at) if kind == "tombstone_rows" else self.ix.tombstone_mask(mk["h"])
                if got != want:
                    self.fail("%s dropped %d, model %d" % (kind, got, want))
        self.live[at] = False
        self.check_state()
        return True

    def op_move(self, kind):
        from syzgydb_amd import _lib
        n = len(self.rows)
        alive = np.flatnonzero(self.live)
        if alive.size == 0:
            return False
        if kind == "compact":
            src = alive
        else:
            src = self.rng.permutation(alive)[: int(self.rng.integers(1, alive.size + 1))]
        moves = kind == "reorder" or alive.size < n
        cols = [c for c in (self.fcol, self.tcol) if c is not None and len(c["pres"]) == n]
        carry_m = [m for m in self.current() if self.rng.random() < 0.6]
        carry_c = [c for c in cols if self.rng.random() < 0.6]
        self.note("%s %s carry masks %s columns %s" % (kind, "" if kind == "compact" else (src + self.base).tolist(),
                                                       [m["id"] for m in carry_m], [c["name"] for c in carry_c]))
        if self.ix is not None:
            carry = [m["h"] for m in carry_m] + [c["h"] for c in carry_c]
            if kind == "compact":
                want = np.full(n, U64_MAX, dtype=np.uint64)
                want[alive] = np.arange(alive.size, dtype=np.uint64) + np.uint64(self.base)
                got = self.ix.compact(carry=carry)
                if not (got == want).all():
                    self.fail("compact: new_of_old differs at rows %s" % np.flatnonzero(got != want)[:8])
            else:
                self.ix.reorder((src + self.base).astype(np.uint64), carry=carry)
        if moves:
            self.rows, self.live = self.rows[src].copy(), np.ones(src.size, dtype=bool)
            self.shards = self.split(src.size)
            for m in carry_m:
                m["arr"] = m["arr"][src]
            for c in carry_c:
                c["pres"] = c["pres"][src]
                c["vals"] = c["vals"][src] if isinstance(c["vals"], np.ndarray) else [c["vals"][i] for i in src]
            q = np.zeros(self.dim)
            for m in [m for m in self.masks if not any(m is x for x in carry_m)]:   # stale: refused on use, then dropped
                if self.ix is not None:
                    self.refused(lambda: self.ix.search_topk(q, 1, masks=m["h"]), _lib.SZG_E_INVALID, "stale mask")
                self.drop_mask(m)
            for c in [c for c in (self.fcol, self.tcol) if c is not None and not any(c is x for x in carry_c)]:
                if self.ix is not None:
                    self.refused(lambda: c["h"].present(), _lib.SZG_E_INVALID, "stale column")
                    c["h"].close()
                if c["name"] == "f64":
                    self.fcol = None
                else:
                    self.tcol = None
        self.check_state()
        for m in carry_m:
            self.check_mask(m)
        for c in carry_c:
            self.check_column(c)
        return True

    # -- masks --------------------------------------------------------------------------------------------------------------
    def drop_mask(self, m):
        if m["h"] is not None:
            m["h"].close()
        self.masks = [x for x in self.masks if x is not m]

    def new_mask(self, arr, make, how):
        self.mask_no += 1
        m = dict(id=self.mask_no, arr=np.asarray(arr, dtype=bool).copy(), stale=False, h=None)
        self.note("  mask %d = %s (%d rows allowed)" % (m["id"], how, int(m["arr"].sum())))
        if self.ix is not None:
            m["h"] = make()
        self.masks.append(m)
        self.check_mask(m)
        if len(self.masks) > 8:
            self.drop_mask(self.masks[0])
        return m

    def check_mask(self, m):
        if self.ix is None:
            return
        if not same_mask(m["h"].read(), m["arr"]):
            self.fail("mask %d: read() differs from the model" % m["id"])
        if m["h"].count != int(m["arr"].sum()):
            self.fail("mask %d: count %d, model %d" % (m["id"], m["h"].count, int(m["arr"].sum())))

    def a_mask(self, sparse=False):
        """A current mask of the model; a new one where there is none (or none sparse enough for a delete)."""
        have = self.current()
        if sparse:
            have = [m for m in have if (m["arr"] & self.live).sum() * 2 <= self.live.sum()]
        if have:
            return self.choice(have)
        arr = self.rng.random(len(self.rows)) < (0.1 if sparse else float(self.choice([0.05, 0.5, 0.95])))
        return self.new_mask(arr, lambda: self.ix.mask(arr), "mask(bool)")

    def op_mask(self, kind):
        n = len(self.rows)
        if kind in ("mask_count", "mask_read"):   # stale masks can still be read and counted
            if not self.masks:
                return False
            m = self.choice(self.masks)
            self.note("%s mask %d%s" % (kind, m["id"], " (stale)" if m["stale"] else ""))
            self.check_mask(m)
            return True
        if kind in ("mask_bool", "mask_words", "mask_rows"):
            self.note(kind)
            if kind == "mask_rows":
                at = self.rng.integers(0, n, int(self.choice([0, 1, 5, 70]))).astype(np.uint64)
                arr = np.zeros(n, dtype=bool)
                arr[at.astype(np.int64)] = True
                self.new_mask(arr, lambda: self.ix.mask_rows(at + np.uint64(self.base)), "mask_rows(%s)" % (at + np.uint64(self.base)).tolist())
            else:
                arr = self.rng.random(n) < float(self.choice([0.0, 0.05, 0.5, 0.95, 1.0]))
                words = pack_bits(arr)
                self.new_mask(arr, lambda: self.ix.mask(arr if kind == "mask_bool" else words), "%s density %.2f" % (kind, arr.mean()))
            return True
        have = self.current()
        if not have:
            return False
        a, b = self.choice(have), self.choice(have)
        self.note("%s of masks %d, %d" % (kind, a["id"], b["id"]))
        if kind == "mask_and":
            self.new_mask(a["arr"] & b["arr"], lambda: a["h"] & b["h"], "%d & %d" % (a["id"], b["id"]))
        elif kind == "mask_or":
            self.new_mask(a["arr"] | b["arr"], lambda: a["h"] | b["h"], "%d | %d" % (a["id"], b["id"]))
        elif kind == "mask_andnot":
            self.new_mask(a["arr"] & ~b["arr"], lambda: a["h"].andnot(b["h"]), "%d &~ %d" % (a["id"], b["id"]))
        else:
            self.new_mask(~a["arr"], lambda: ~a["h"], "~%d" % a["id"])
        return True

    # -- columns ------------------------------------------------------------------------------------------------------------
    def text_values(self, m):
        out = []
        for _ in range(m):
            ln = int(self.rng.integers(0, 5))
            out.append(b"".join(ALPHABET[int(i)] for i in self.rng.integers(0, len(ALPHABET), ln)))
        return out

    def column_values(self, name, m):
        pres = self.rng.random(m) < 0.8
        if name == "f64":
            return FVALS[self.rng.integers(0, FVALS.size, m)], pres
        return self.text_values(m), pres

    def check_column(self, c):
        if self.ix is None:
            return
        vals, pres = c["h"].read()
        if not same_column(vals, pres, c["vals"], c["pres"]):
            self.fail("column %s: read() differs from the model" % c["name"])

    def op_column(self, kind):
        n = len(self.rows)
        if kind == "col_new":
            free = [name for name, c in (("f64", self.fcol), ("text", self.tcol)) if c is None]
            if not free:
                return False
            name = self.choice(free)
            vals, pres = self.column_values(name, n)
            c = dict(name=name, vals=vals, pres=pres, h=None)
            self.note("col_new %s over %d rows" % (name, n))
            self.count("col_new:%s" % name)
            if self.ix is not None:
                # (a text value of an absent row is kept out of the heap: None)
                c["h"] = self.ix.column(vals, present=pres) if name == "f64" else self.ix.text_column(vals, present=pres)
            if name == "f64":
                self.fcol = c
            else:
                self.tcol = c
            self.check_column(c)
            return True
        if kind == "col_append":
            short = [c for c in (self.fcol, self.tcol) if c is not None and len(c["pres"]) < n]
            if not short:
                return False
            c = self.choice(short)
            m = n - len(c["pres"])
            vals, pres = self.column_values(c["name"], m)
            self.note("col_append %s %d rows" % (c["name"], m))
            if self.ix is not None:
                c["h"].append(vals, present=pres)
            c["pres"] = np.concatenate([c["pres"], pres])
            c["vals"] = np.concatenate([c["vals"], vals]) if c["name"] == "f64" else c["vals"] + vals
            self.check_column(c)
            return True
        c = self.fcol if kind == "col_set_rows" else self.tcol
        if c is None or len(c["pres"]) == 0:
            return False
        have = len(c["pres"])
        if kind == "col_set_rows":
            at = self.rng.choice(have, size=min(have, int(self.choice([1, 4, 60]))), replace=False)
            vals, pres = self.column_values("f64", at.size)
            self.note("col_set_rows %s values %s present %s" % ((at + self.base).tolist(), vals.tolist(), pres.astype(int).tolist()))
            if self.ix is not None:
                c["h"].set_rows((at + self.base).astype(np.uint64), vals, present=pres)
            c["pres"][at] = pres
            c["vals"][at[pres]] = vals[pres]
        else:
            at = int(self.rng.integers(0, have))
            val = None if self.rng.random() < 0.2 else self.text_values(1)[0]
            self.note("col_set text row %d = %r" % (at + self.base, val))
            if self.ix is not None:
                c["h"].set(at + self.base, val)
            c["pres"][at] = val is not None
            if val is not None:
                c["vals"][at] = val
        self.check_column(c)
        return True

    def op_where(self, kind):
        n = len(self.rows)
        c = self.fcol if kind in ("where", "isin", "present") and not (kind == "present" and self.rng.random() < 0.3) else self.tcol
        if c is None or len(c["pres"]) != n:
            return False
        base = self.a_mask() if self.rng.random() < 0.5 else None
        bh = None if base is None else base["h"]
        how = "%s.%s" % (c["name"], kind)
        if kind == "where":
            op, const = self.choice(list(CMP)), float(self.choice(FVALS))
            with np.errstate(invalid="ignore"):
                arr = CMP[op](c["vals"], const)
            how += " %s %r" % (op, const)
            self.count("where:%s" % op)
            make = lambda: c["h"].where(op, const, base=bh)   # noqa: E731
        elif kind == "isin":
            consts = FVALS[self.rng.integers(0, FVALS.size, int(self.choice([0, 1, 3])))]
            arr = (c["vals"][:, None] == consts[None, :]).any(axis=1)
            how += " %s" % consts.tolist()
            make = lambda: c["h"].isin(consts, base=bh)   # noqa: E731
        elif kind == "present":
            arr = np.ones(n, dtype=bool)
            make = lambda: c["h"].present(base=bh)   # noqa: E731
        else:
            const = self.choice(c["vals"])[: int(self.rng.integers(0, 4))] if n and self.rng.random() < 0.7 else self.text_values(1)[0]
            how += " %r" % const
            if kind == "startswith":
                arr = np.array([v.startswith(const) for v in c["vals"]], dtype=bool)
                make = lambda: c["h"].startswith(const, base=bh)   # noqa: E731
            elif kind == "contains":
                arr = np.array([const in v for v in c["vals"]], dtype=bool)
                make = lambda: c["h"].contains(const, base=bh)   # noqa: E731
            else:
                arr = np.array([v == const for v in c["vals"]], dtype=bool)
                make = lambda: c["h"].eq(const, base=bh)   # noqa: E731
        arr = arr.reshape(n) & c["pres"]
        if base is not None:
            arr = arr & base["arr"]
            how += " base %d" % base["id"]
        self.note(kind)
        self.count("base:%s" % ("with" if base is not None else "without"))
        self.new_mask(arr, make, how)
        return True

    # -- questions ----------------------------------------------------------------------------------------------------------
    def queries(self, nq, dt):
        orc = self.fz.orc
        Q = self.rng.uniform(-1, 1, (nq, self.dim))
        n = len(self.rows)
        for qj in range(nq):
            if self.near.random() >= 0.2:
                continue
            x = orc.decode_vector(self.rows[int(self.near.integers(0, n))], self.dim, self.bits)   # a stored row ...
            if self.near.random() < 0.5:   # ... or one moved by a few spacings (fuzz_gpu.py's construction)
                g = x * (65535.0 if self.bits == 16 else 1.0)
                sp = np.spacing(np.abs(g).astype(np.float32)).astype(np.float64) / (65535.0 if self.bits == 16 else 1.0)
                if self.bits <= 8:
                    sp = np.full(self.dim, np.abs(x).max() / float(self.near.choice([16000.0, 30000.0, 1000000.0])))
                move = float(self.near.choice([0.25, 0.25, 1.0, 3.0, 17.0]))
                at = self.near.random(self.dim) < float(self.near.choice([0.1, 1.0]))
                at[int(self.near.integers(0, self.dim))] = True
                step = self.near.uniform(-1, 1, self.dim) if move < 1 else self.near.choice((-1.0, 1.0), self.dim)
                x = x + at * step * move * sp
            Q[qj] = x
        return round_to(Q, dt)

    def collect_served(self, k, nq):
        if self.opts.get("sketch_topk_collect") != 1 or k < 35:
            return False
        planes = 3 if self.opts.get("sketch_planes") == 3 else 2   # (the plan is the 8-bit sketch's; it wants two planes)
        nq = min(nq, 32)   # (the plan is per launch: at most 32 queries per row read)
        return all(self.fz.sample_plan(s, k, nq, self.dim, 8, planes)["serves"] for s in self.shards if s) and any(self.shards)

    def op_search(self, kind):
        orc, rng = self.fz.orc, self.rng
        n = len(self.rows)
        tensor = kind.endswith("_tensor")
        topk = "topk" in kind
        lone = kind in ("search_radius", "search_radius_capacity")
        nq = 1 if lone else int(self.choice(NQS))
        dt = self.choice(DTYPES)
        self.count("%s:%s" % (kind, dt))
        k = int(self.choice(KS))
        if topk and self.fz.profile == "sketched":   # a k that the soaking paths serve, more often than the list gives it
            served = [x for x in KS if self.collect_served(x, nq)]
            if served and rng.random() < 0.7:
                k = int(self.choice(served))
            elif self.opts.get("sketch_masked") == 1 and rng.random() < 0.5:
                k = int(self.choice([1, 10, 34]))
        if tensor:   # (the tensor calls take resident masks only, a truncated answer host words only)
            filt = self.choice(["none", "shared", "each"])
        elif kind == "search_radius_capacity":
            filt = self.choice(["none", "allow"])
        else:
            filt = self.choice(["none", "allow", "shared"] if lone else ["none", "none", "allow", "shared", "each"])
        src = None
        if tensor and rng.random() < 0.5:   # the queries are listed rows of a pool, duplicates allowed
            pool = self.queries(int(rng.integers(1, nq + 3)), dt)
            src = rng.integers(0, len(pool), nq)
            Q = pool[src]
        else:
            pool = Q = self.queries(nq, dt)
        if filt == "allow":
            allow = rng.random((nq, n)) < float(self.choice([0.05, 0.5, 0.95]))
            F = list(allow)
            as_words = rng.random() < 0.5   # the caller's own uint64 words, or booleans that the wrapper packs
            self.count("allow:%s" % ("words" if as_words else "bool"))
        elif filt == "shared":
            mk = [self.a_mask()]
            F = [mk[0]["arr"]] * nq
        elif filt == "each":
            mk = [None if rng.random() < 0.3 else self.a_mask() for _ in range(nq)]
            F = [None if m is None else m["arr"] for m in mk]
        else:
            F = [None] * nq
        elig = [(self.live if f is None else self.live & f).astype(np.uint8) for f in F]
        if topk:
            if self.opts.get("sketch_masked") == 1 and (filt != "none" or not self.live.all()):
                self.count("coincide:sketch_masked")
            if self.collect_served(k, nq):
                self.count("coincide:sketch_topk_collect")
            want = [orc.search_exact(self.rows, self.dim, self.bits, self.metric, Q[i], k=k, allow=elig[i])[:2] for i in range(nq)]
            radii = None
        else:
            radii = []
            for i in range(nq):
                od = orc.search_exact(self.rows, self.dim, self.bits, self.metric, Q[i], k=int(self.choice([1, 5, 20, 60])), allow=elig[i])[1]
                fin = [x for x in od if x == x and x > 0]
                radii.append(float(fin[-1]) if fin else 0.5)
            want = [orc.search_exact(self.rows, self.dim, self.bits, self.metric, Q[i], radius=radii[i], allow=elig[i])[:2] for i in range(nq)]
        cap = None
        if kind == "search_radius_capacity":
            if len(want[0][0]) < 2:
                return False
            cap = int(rng.integers(1, len(want[0][0])))
        elif not topk and not lone and rng.random() < 0.3:
            cap = 1   # the first attempt is too small: the batch is answered a second time
        self.note("%s nq %d dtype %s%s filter %s%s%s%s queries %s" % (
            kind, nq, dt, " k %d" % k if topk else " radii %r" % radii, filt + (" (words)" if filt == "allow" and as_words else ""),
            " masks %s" % [None if m is None else m["id"] for m in mk] if filt in ("shared", "each") else "",
            " src_rows %s of %d" % (src.tolist(), len(pool)) if src is not None else "", " capacity %s" % cap if cap else "",
            [float(x) for x in Q[0][:4]]))
        if self.ix is None:
            return True
        ix = self.ix
        fargs = {}
        if filt == "allow":
            fargs = dict(allow=np.stack([pack_bits(a) for a in allow]) if as_words else allow)
        elif filt == "shared":
            fargs = dict(masks=mk[0]["h"])
        elif filt == "each":
            fargs = dict(masks=[None if m is None else m["h"] for m in mk])
        total = None
        if kind == "search_topk":
            r, d, c = ix.search_topk(Q, k, **fargs)
        elif kind == "search_topk_tensor":
            r, d, c = ix.search_topk_tensor(self.card.tensor(pool, dt), k, src_rows=src, **fargs)
        elif kind == "search_radius":
            got = [ix.search_radius(Q[0], radii[0], **fargs)]
        elif kind == "search_radius_capacity":
            tr, td, total = ix.search_radius(Q[0], radii[0], capacity=cap, **fargs)
            got = [(tr, td)]
        elif kind == "search_radius_batch":
            got = ix.search_radius_batch(Q, radii, capacity=cap, **fargs)
        else:
            got = ix.search_radius_tensor(self.card.tensor(pool, dt), radii, src_rows=src, capacity=cap, **fargs)
        if topk:
            got = [(r[i, : c[i]], d[i, : c[i]]) for i in range(nq)]
        if total is not None:
            if total != len(want[0][0]):
                self.fail("%s: total %d, oracle %d" % (kind, total, len(want[0][0])))
            want = [(want[0][0][:cap], want[0][1][:cap])]
        for i in range(nq):
            wr = want[i][0] + np.uint64(self.base)
            if not same_answer(got[i][0], got[i][1], wr, want[i][1], live=self.live, base=self.base):
                self.fail("%s query %d\n  got  %s %s\n  want %s %s" % (kind, i, [int(x) for x in got[i][0][:12]], got[i][1][:6],
                                                                      [int(x) for x in wr[:12]], want[i][1][:6]))
        self.certificates(Q, np.array(elig, dtype=bool), kind, radii)
        return True

    def certificates(self, Q, eligible, call, radii):
        """--certificates: the records of the call just made, checked as fuzz_gpu.py checks them."""
        if not self.fz.args.certificates:
            return
        from syzgydb_amd import cert_check
        orc, ix = self.fz.orc, self.ix
        recs, ents, dropped = ix.certificates()
        if self.base:   # (read and dropped: the checker numbers rows from 0)
            return
        recs = recs.copy()
        corpus = cert_check.Corpus(self.rows, self.dim, self.bits, self.metric)
        dists = sketch = None
        if np.isin(recs["pass_"], (1, 5, 6)).any():
            dists = np.stack([orc.all_distances(self.rows, self.dim, self.bits, self.metric, q) for q in Q])
            info = ix.sketch_info()
            if info["exists"] and info["in_sync"]:
                sketch = (cert_check.Corpus(ix.sketch_rows()[0], self.dim, 8, self.metric), info["gscale"], info["exc_rows"])
        try:
            cert_check.check(corpus, Q, recs, ents, dropped, eligible=eligible, dists=dists, what=(call,), sketch=sketch, radii=radii)
            cert_check.check_bf16_tight(corpus, Q, recs, ents, what=(call,))
        except AssertionError as e:
            self.fail("certificate of %s: %s" % (call, str(e)[:600]))

    # -- readers ------------------------------------------------------------------------------------------------------------
    def op_fetch(self, kind):
        n = len(self.rows)
        dt = self.choice(DTYPES)
        self.count("%s:%s" % (kind, dt))
        off = int(self.rng.integers(0, 2))   # aligned, or one element further on
        if kind == "fetch_range":
            first = int(self.rng.integers(0, n))
            at = np.arange(first, first + int(self.rng.integers(1, n - first + 1)))
        else:
            at = self.rng.integers(0, n, int(self.choice([1, 9, 70, 300])))
        self.note("%s dtype %s offset %d rows %s" % (kind, dt, off, ("%d..%d" % (at[0] + self.base, at[-1] + self.base))
                                                     if kind == "fetch_range" else (at + self.base).tolist()))
        if self.ix is None:
            return True
        torch = self.card.torch
        flat = torch.full((at.size * self.dim + off,), 7.0, dtype=self.card.types[dt], device="cuda")
        out = flat[off:].view(at.size, self.dim)
        if kind == "fetch_range":
            self.ix.fetch_into(out, first_row=int(at[0]) + self.base, n_rows=at.size)
        else:
            self.ix.fetch_into(out, rows=(at + self.base).astype(np.uint64))
        want = self.card.chain(self.fz.codec.decode_rows(self.rows[at], self.dim, self.bits), dt)
        if not same_tensor_bits(self.card.bits(out), want):
            self.fail("%s: the fetched tensor differs from the cast chain" % kind)
        if off and float(flat[0]) != 7.0:
            self.fail("%s: the element before the destination was written" % kind)
        return True

    def op_distances(self, kind):
        orc = self.fz.orc
        n = len(self.rows)
        if kind == "distances":
            q = self.queries(1, self.choice(DTYPES))[0]
            pick = self.rng.integers(0, n, min(n, 40))
            self.note("distances rows %s query %s" % ((pick + self.base).tolist(), [float(x) for x in q[:4]]))
            want = orc.all_distances(self.rows[pick], self.dim, self.bits, self.metric, q)
            got = None if self.ix is None else self.ix.distances(q, (pick + self.base).astype(np.uint64))
        else:
            pa, pb = self.rng.integers(0, n, 20), self.rng.integers(0, n, 20)
            self.note("pair_distances %s %s" % ((pa + self.base).tolist(), (pb + self.base).tolist()))
            fn = orc.angular if self.metric == 1 else orc.euclidean
            want = np.array([fn(orc.decode_vector(self.rows[x], self.dim, self.bits), orc.decode_vector(self.rows[y], self.dim, self.bits))
                             for x, y in zip(pa, pb)])
            got = None if self.ix is None else self.ix.pair_distances((pa + self.base).astype(np.uint64), (pb + self.base).astype(np.uint64))
        if got is not None and not same_answer(np.zeros(len(want)), got, np.zeros(len(want)), want):
            self.fail("%s differ from the oracle" % kind)
        return True

    # -- refusals the model predicts ----------------------------------------------------------------------------------------
    def op_refusal(self, kind):
        from syzgydb_amd import _lib
        n = len(self.rows)
        ix = self.ix
        if kind == "refuse_stale_mask":
            stale = [m for m in self.masks if m["stale"]]
            if not stale:
                return False
            m = self.choice(stale)
            how = self.choice(["search_topk", "search_radius_batch", "combine", "tombstone_mask"])
            self.note("refuse_stale_mask %d in %s" % (m["id"], how))
            if ix is not None:
                q = np.zeros(self.dim)
                call = {"search_topk": lambda: ix.search_topk(q, 1, masks=m["h"]),
                        "search_radius_batch": lambda: ix.search_radius_batch(q, 0.5, masks=m["h"]),
                        "combine": lambda: ~m["h"], "tombstone_mask": lambda: ix.tombstone_mask(m["h"])}[how]
                self.refused(call, _lib.SZG_E_INVALID, "stale mask")
        elif kind == "refuse_short_column":   # a column the appends left short: no where-mask until it is level
            short = [c for c in (self.fcol, self.tcol) if c is not None and len(c["pres"]) < n]
            if not short:
                return False
            c = self.choice(short)
            how = self.choice(["present", "where"])
            self.note("refuse_short_column %s (%d of %d rows) in %s" % (c["name"], len(c["pres"]), n, how))
            if ix is not None:
                const = 1.5 if c["name"] == "f64" else b"a"
                call = (lambda: c["h"].present()) if how == "present" else (lambda: c["h"].where("==", const))
                self.refused(call, _lib.SZG_E_INVALID, "short column")
        elif kind == "refuse_twice":
            at = self.rng.integers(0, n, int(self.choice([1, 3, 30])))
            at = np.concatenate([at, at[:1]]).astype(np.uint64)
            how = self.choice(["overwrite_rows", "overwrite_vectors"])
            v = self.vectors(at.size)
            self.note("refuse_twice %s %s" % (how, at.tolist()))
            if ix is not None:
                call = (lambda: ix.overwrite_rows(at, self.encode(v))) if how == "overwrite_rows" else (lambda: ix.overwrite_vectors(at, v))
                self.refused(call, _lib.SZG_E_INVALID, "row listed twice")
        else:
            how = self.choice(["overwrite_rows", "tombstone_rows", "mask_rows", "overwrite"])
            at = np.concatenate([self.rng.choice(n, size=min(n, 3), replace=False), [n]]).astype(np.uint64)
            new = self.encode(self.vectors(at.size))   # (drawn here: no draw may depend on whether a card is used)
            self.note("refuse_range %s %s" % (how, at.tolist()))
            if ix is not None:
                call = {"overwrite_rows": lambda: ix.overwrite_rows(at, new),
                        "tombstone_rows": lambda: ix.tombstone_rows(at),
                        "mask_rows": lambda: ix.mask_rows(at + np.uint64(self.base)),
                        "overwrite": lambda: ix.overwrite(n, new[0])}[how]
                self.refused(call, _lib.SZG_E_RANGE, "out of range")
        self.check_state()   # nothing changed
        return True


class Fuzzer:
    def __init__(self, args):
        import oracle
        from syzgydb_amd import codec, scan_lattice
        from syzgydb_amd.index import sample_plan
        self.args, self.profile = args, args.profile
        self.orc, self.codec, self.lattice, self.sample_plan = oracle, codec, scan_lattice, sample_plan
        self.card = None if args.plan_only else Card()
        self.counts, self.served, self.failures = {}, {}, 0
        self.digest = hashlib.sha256()   # of every case's operation log

    def collect(self, ix, bits):
        """The path counters of a handle about to close, summed into `served`."""
        st = ix.stats()
        add = {name: int(st[name]) for name in SERVED}
        add["sketch_topk_collect_queries"] = ix.sketch_topk_stats()["queries"]
        add["sketch_masked_launches"] = ix.sketch_masked_info()["launches"]
        for name, val in ix.mask_stats().items():
            if name in ("h2d_bytes", "d2d_bytes", "shared_batches"):
                add["mask_" + name] = val
        add["sketch_queries_64bit"] = (add["sketch_queries"] + add["sketch_radius_queries"] +
                                       add["sketch_topk_collect_queries"]) if bits == 64 else 0
        for name, val in add.items():
            self.served[name] = self.served.get(name, 0) + int(val)

    def run(self):
        for no in range(1, self.args.cases + 1):
            case = Case(self, no)
            try:
                case.run()
            except Mismatch as e:
                self.failures += 1
                print("MISMATCH %s" % e, flush=True)
                print("\n".join(case.log), flush=True)
            except Exception as e:  # noqa: BLE001 -- not predicted by the model: nothing more is started on the card
                print("UNEXPECTED %r" % (e,), flush=True)
                print("\n".join(case.log), flush=True)
                print(json.dumps(self.result(no, fatal=repr(e))), flush=True)
                return 2
            self.digest.update("\n".join(case.log).encode())
            if self.args.plan_only:
                print("\n".join(case.log), flush=True)
            if no % 25 == 0:
                print("cases %d, failures %d" % (no, self.failures), flush=True)
        print(json.dumps(self.result(self.args.cases)), flush=True)
        return 1 if self.failures else 0

    def result(self, cases, **more):
        return dict(seed=self.args.seed, profile=self.profile, cases=cases, failures=self.failures,
                    operations=dict(sorted(self.counts.items())), plan=self.digest.hexdigest(), served=self.served, **more)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("seed", type=int)
    ap.add_argument("--cases", type=int, required=True, help="run exactly this many cases")
    ap.add_argument("--profile", choices=("plain", "sketched"), default="plain")
    ap.add_argument("--plan-only", action="store_true", help="generator, model and oracle only: print the plan, touch no card")
    ap.add_argument("--certificates", action="store_true", help="check every search's certificate trace against float64")
    return Fuzzer(ap.parse_args(argv)).run()


if __name__ == "__main__":
    sys.exit(main())
