"""Host-side mirror of the reference's Collection API for the search path.

Same names, argument meaning and error behaviour as collection.go:
CollectionOptions (:31-48), Document (:100-110), SearchArgs (:140-158),
SearchResult/SearchResults (:115-135), Collection.AddDocument (:427-457),
GetDocument (:463-484), UpdateDocument (:490-509), removeDocument (:511-521),
Search (:569-711).  What differs is only WHERE the exact scan runs: the HOT
LOOP (:672-684) is one call through the C ABI into the HIP library.

Storage, the LSH index, REST, and the filter language stay in the reference
and are out of scope here: documents live in host memory, and any Precision
is answered by the exact scan (the reference's LSH path is unchanged Go code).
"""
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np

from . import _lib, codec, regex_dfa as _regex_dfa, where as _where
from .index import ScanIndex, pack_allow_bits

Euclidean = 0  # collection.go:186-189
Cosine = 1


@dataclass
class CollectionOptions:
    """collection.go:31-48."""
    Name: str = ""
    DistanceMethod: int = Euclidean
    DimensionCount: int = 0
    Quantization: int = 0  # 0 -> 64, as NewCollection does (collection.go:254-256)


@dataclass
class Document:
    ID: int
    Vector: np.ndarray
    Metadata: bytes


@dataclass
class SearchResult:
    ID: int
    Metadata: bytes
    Distance: float = 0.0


@dataclass
class SearchResults:
    Results: List[SearchResult] = field(default_factory=list)
    PercentSearched: float = 0.0


@dataclass
class SearchArgs:
    """collection.go:140-158."""
    Vector: Optional[np.ndarray] = None
    Filter: Optional[Callable[[int, bytes], bool]] = None
    K: int = 0
    Radius: float = 0.0
    Offset: int = 0
    Limit: int = 0
    Precision: str = ""
    FilterKey: Optional[str] = None  # not in the reference: names the filter for the bitmask cache
    Where: Optional[object] = None   # not in the reference: the filter as a where.Expr (exclusive with Filter); fields
                                     # indexed with Collection.IndexField are compared on the card


class _FieldIndex:
    """One indexed metadata field: its column on the card and, for kind "string", the dictionary value -> code."""

    def __init__(self, name, kind):
        self.name = name
        self.kind = kind        # "number" / "string" / "text"
        self.column = None      # ScanColumn
        self.codes = {}         # string fields: value -> code, append-only, first-seen order

    def value_of(self, data):
        """(value, present) of one document for the column: data = its parsed metadata (None: not a JSON object)."""
        v = data.get(self.name) if data is not None else None
        if self.kind == "number":
            if _where._is_number(v):
                return _where._number(v), True
            return 0.0, False
        if self.kind == "text":
            return (v, True) if isinstance(v, str) else (None, False)
        if isinstance(v, str):
            return self.codes.setdefault(v, len(self.codes)), True
        return 0, False


class Collection:
    def __init__(self, options: CollectionOptions, devices=None, sketch=None, strict_order=True, auto_compact=None):
        if options.Quantization == 0:
            options.Quantization = 64  # collection.go:254-256
        if options.DistanceMethod not in (Euclidean, Cosine):
            raise ValueError("unsupported distance method")  # collection.go:282
        codec.vector_size(options.Quantization, options.DimensionCount)  # panics like :809
        self.options = options
        self.DimensionCount = options.DimensionCount
        self.Quantization = options.Quantization
        self.DistanceMethod = options.DistanceMethod
        self._index = ScanIndex(self.DimensionCount, self.Quantization, self.DistanceMethod,
                                devices=devices)
        if sketch is not None:
            # 8-bit sketch pre-pass for lone Searches on float32 collections (same answers, +25 % device memory):
            # None = the library's default (automatic), True / False force it on / off
            self._index.set_option("sketch", 1 if sketch else 0)
            # ... and, forced on, for lone radius Searches too (option sketch_radius, off by default)
            self._index.set_option("sketch_radius", 1 if sketch else 0)
        # removeDocument only tombstones a row: its bytes stay on the card and are swept by every search until
        # Compact() drops them.  auto_compact = a fraction f: removeDocument compacts by itself once the tombstoned
        # rows exceed f of the mirror's rows; None (the default) = never
        if auto_compact is not None and not 0.0 <= float(auto_compact) < 1.0:
            raise ValueError("auto_compact is None or a fraction in [0, 1)")
        self.auto_compact = None if auto_compact is None else float(auto_compact)
        self.compactions = 0
        self.column_rebuilds = 0   # calls of _rebuild_columns (the columns made again from the metadata); the package itself makes none
        self._row_of = {}    # id -> row
        self._id_of = []     # row -> id (None once tombstoned)
        self._meta = []      # row -> metadata bytes
        self._closed = False
        # filter -> allow-bitmask cache: a filter's verdicts only change when the
        # collection does, so they are kept per (filter key, collection version) -- the host words and, beside them,
        # the ScanMask that holds the same bits on the card: searches pass the handle, nothing is uploaded again
        self._version = 0
        self._mask_cache = {}   # (key, version) -> [words, filter, ScanMask or None]
        # metadata fields resident on the card (IndexField): name -> _FieldIndex, and beside them the hidden column
        # "the metadata is a JSON object" (code 1 / 0), which exists once any field is indexed
        self._fields = {}
        self._object_col = None
        self.where_compiled = 0    # Where expressions turned into a mask through the columns
        self.where_fallbacks = 0   # ... answered through the Filter path (a field not indexed, a constant of another type)
        # Row order only matters where the reference's own answer depends on its visit order: ties at the k
        # boundary, equal distances in a radius result (collection.go:608).  Production iterates a Go map (random
        # order per run, spanfile.go:525): every order is a reference order, rows are simply appended
        # (strict_order=False).  The reference's deterministic mode (seeded tests, spanfile.go:522) pins the order
        # to sort.Strings of the decimal ids; that is what the parity tests compare with, hence the default.  A new
        # id is ALWAYS appended in place; one that sorts before the last ("10" < "9": ordinary ascending integers
        # do that) only marks the order stale, and the mirror is re-paged in order the first time an answer
        # actually contains such a tie -- not on every add (the same rule as go/syzgy_gpu.go).
        self.strict_order = bool(strict_order)
        self._last_idstr = ""
        self._order_stale = False
        self.resorts = 0

    @classmethod
    def from_spanfile(cls, path, devices=None):
        """Open an existing SyzgyDB collection file: the header record's options
        override the caller's (collection.go:241-252), every record's packed vector
        is paged into HBM in IterateSortedRecords order (collection.go:297-311)."""
        from .pager import SpanfilePager
        with SpanfilePager(path) as pg:
            c = cls(CollectionOptions(Name=str(path), DistanceMethod=pg.metric,
                                      DimensionCount=pg.dim, Quantization=pg.quant_bits),
                    devices=devices)
            pg.load_into(c._index)
            for row, id in enumerate(pg.ids()):
                c._row_of[int(id)] = row
                c._id_of.append(int(id))
                c._meta.append(pg.metadata(row))
                c._last_idstr = str(int(id))
        return c

    def _note_appended(self, id):
        """Row order bookkeeping for a new id appended at the end of the mirror."""
        s = str(id)
        if s < self._last_idstr:
            self._order_stale = self.strict_order
        else:
            self._last_idstr = s

    def _resort(self):
        """Re-page the live rows in sorted decimal-string id order: the rows are reordered on the card
        (ScanIndex.reorder), nothing travels through the host, and the resident columns follow their rows there.  No
        mask is carried: the numbering changes arbitrarily, and the version moves."""
        live = sorted((str(id), id, row) for id, row in self._row_of.items())
        rows = [row for _, _, row in live]
        new_meta = [self._meta[r] for r in rows]
        self._index.reorder(np.asarray(rows, dtype=np.uint64), carry=self._resident_columns())
        self._id_of = [id for _, id, _ in live]
        self._meta = new_meta
        self._row_of = {id: i for i, id in enumerate(self._id_of)}
        self._last_idstr = live[-1][0] if live else ""
        self._order_stale = False
        self.resorts += 1
        self._version += 1  # rows are renumbered: cached filter masks no longer apply

    # -- CRUD (host bookkeeping + mirror maintenance) ---------------------------
    def AddDocument(self, id: int, vector, metadata: bytes = b""):
        v = np.asarray(vector, dtype=np.float64).reshape(-1)
        if v.size != self.DimensionCount:
            # log.Panicf in the reference (collection.go:432-434)
            raise ValueError("vector size does not match the expected number of dimensions: "
                             "expected %d, got %d" % (self.DimensionCount, v.size))
        row_bytes = codec.encode_rows(v.reshape(1, -1), self.Quantization)
        id = int(id)
        self._version += 1
        if id in self._row_of:  # WriteRecord of an existing id replaces the record
            row = self._row_of[id]
            self._index.overwrite(row, row_bytes)
            self._meta[row] = bytes(metadata)
            self._columns_set(row)
        else:
            self._index.append(row_bytes)
            self._row_of[id] = len(self._id_of)
            self._id_of.append(id)
            self._meta.append(bytes(metadata))
            self._note_appended(id)
            self._columns_append(1)

    def AddDocuments(self, ids, vectors, metadatas=None):
        """Bulk upsert (not in the reference; the same state as AddDocument in a loop over the entries): new ids are
        appended by ONE append_vectors in first-seen order, existing ids rewritten by ONE overwrite_vectors -- both
        quantize and pack on the device.  An id listed twice keeps its last entry.
        vectors may also lie in device memory -- a torch tensor on the card, or any object with
        __cuda_array_interface__ (ScanIndex.append_tensor) -- and then never visit the host: the two lists of entries
        become the src_rows of one overwrite_tensor and one append_tensor."""
        on_device = bool(getattr(vectors, "is_cuda", False)) or (hasattr(vectors, "__cuda_array_interface__") and
                                                                 not hasattr(vectors, "data_ptr"))
        if on_device:
            V = None
            width = tuple(vectors.shape)[1] if len(tuple(vectors.shape)) == 2 else -1
        else:
            V = np.atleast_2d(np.asarray(vectors, dtype=np.float64))
            width = V.shape[1]
        if width != self.DimensionCount:
            raise ValueError("vector size does not match the expected number of dimensions")
        ids = [int(i) for i in ids]
        self._version += 1
        last, fresh = {}, []   # id -> its last entry; the new ids in first-seen order
        for j, i in enumerate(ids):
            if i not in last and i not in self._row_of:
                fresh.append(i)
            last[i] = j

        def meta(j):
            return bytes(metadatas[j]) if metadatas else b""

        known = [i for i in last if i in self._row_of]
        if known:  # WriteRecord of an existing id replaces the record
            rows = [self._row_of[i] for i in known]
            if on_device:
                self._index.overwrite_tensor(rows, vectors, src_rows=[last[i] for i in known])  # szg_index_overwrite_rows_dev
            else:
                self._index.overwrite_vectors(rows, V[[last[i] for i in known]])  # szg_index_overwrite_rows_f64
            for i, row in zip(known, rows):
                self._meta[row] = meta(last[i])
            self._columns_set_rows(rows)
        if not fresh:
            return
        # quantize + pack on the device (szg_index_append_f64; szg_index_append_dev for vectors that are there already)
        if on_device:
            self._index.append_tensor(vectors, src_rows=[last[i] for i in fresh])
        else:
            self._index.append_vectors(V if len(fresh) == len(ids) else V[[last[i] for i in fresh]])
        for i in fresh:
            self._row_of[i] = len(self._id_of)
            self._id_of.append(i)
            self._meta.append(meta(last[i]))
            self._note_appended(i)
        self._columns_append(len(fresh))

    def GetDocument(self, id: int) -> Document:
        row = self._row_of.get(int(id))
        if row is None:
            raise KeyError("record not found")  # spanfile.go:516
        data = self._index.read_rows(row, 1)
        vec = codec.decode_rows(data, self.DimensionCount, self.Quantization)[0]
        return Document(ID=int(id), Vector=vec, Metadata=self._meta[row])

    def FetchVectors(self, ids, out):
        """The vector half of GetDocument for many ids, into device memory (not in the reference): row i of the 2-D
        device tensor `out` (ScanIndex.fetch_into) receives the stored vector of ids[i], decoded on the card.  An
        unknown id is GetDocument's error, raised before anything is written.  Returns `out`."""
        rows = []
        for id in ids:
            row = self._row_of.get(int(id))
            if row is None:
                raise KeyError("record not found")  # spanfile.go:516
            rows.append(row)
        return self._index.fetch_into(out, rows=rows)

    def UpdateDocument(self, id: int, new_metadata: bytes):
        row = self._row_of.get(int(id))
        if row is None:
            raise KeyError("record not found")
        self._version += 1
        self._meta[row] = bytes(new_metadata)
        self._columns_set(row)

    def removeDocument(self, id: int):
        row = self._row_of.pop(int(id), None)
        if row is None:
            raise KeyError("record not found")
        self._version += 1
        self._index.tombstone(row)
        self._id_of[row] = None
        self._meta[row] = b""
        self._columns_set(row)
        if self.auto_compact is not None:
            rows = self._index.rows
            if rows - self._index.live_rows > self.auto_compact * rows:
                self.Compact()

    def _removed(self, ids, rows):
        """Host bookkeeping of rows that have just been tombstoned, then the auto_compact rule, once."""
        for i, row in zip(ids, rows):
            del self._row_of[i]
            self._id_of[row] = None
            self._meta[row] = b""
        self._columns_set_rows(rows)
        if self.auto_compact is not None:
            n = self._index.rows
            if n - self._index.live_rows > self.auto_compact * n:
                self.Compact()

    def RemoveDocuments(self, ids) -> int:
        """removeDocument for a list (not in the reference), ONE tombstone_rows: an unknown id raises KeyError before
        anything changes; an id listed twice counts once.  Returns the documents removed."""
        ids = list(dict.fromkeys(int(i) for i in ids))
        if any(i not in self._row_of for i in ids):
            raise KeyError("record not found")
        if not ids:
            return 0
        rows = [self._row_of[i] for i in ids]
        self._version += 1
        dropped = self._index.tombstone_rows(rows)
        self._removed(ids, rows)
        return dropped

    def RemoveWhere(self, where, key=None) -> int:
        """Remove every document the filter accepts (not in the reference): `where` is a where.Expr -- compiled through
        the columns of the indexed fields like SearchArgs.Where -- or a Filter callable, `key` its cache key.  The
        verdicts are a mask on the card (the filter cache's, when a Search has made it already) and ONE tombstone_mask
        applies it there; the dropped rows are read back from the mask's words.  Returns the documents removed."""
        if not self._row_of:
            return 0
        if isinstance(where, _where.Expr):
            mask = self._where_handle(where)
        elif callable(where):
            mask = self._allow_handle(where, key)
        else:
            raise TypeError("RemoveWhere takes a where.Expr or a filter callable")
        bits = np.unpackbits(mask.read().view(np.uint8), bitorder="little")[:len(self._id_of)]
        rows = [int(r) for r in np.flatnonzero(bits) if self._id_of[int(r)] is not None]
        self._version += 1
        dropped = self._index.tombstone_mask(mask)
        self._removed([self._id_of[r] for r in rows], rows)
        return dropped

    def Compact(self) -> int:
        """Drop the tombstoned rows from the card (not in the reference, whose spanfile reclaims space by itself):
        the live rows keep their order, so answers do not change -- the sweeps read fewer bytes, the memory is
        returned, and a shard without tombstones is back on the unmasked fast paths.  The cached filters of the
        current version are carried: their device masks are renumbered on the card, so the next Search with one of
        them costs neither an evaluation of the filter nor an upload.  The columns of the indexed fields are carried
        the same way: the card gathers their values and present bits and repacks the text heaps (which reclaims the
        bytes of dropped rows and of values that were replaced by longer ones); no metadata is parsed again.  Returns
        the rows dropped."""
        dropped = self._index.rows - self._index.live_rows
        if dropped == 0:
            return 0
        for old in [k for k in self._mask_cache if k[1] != self._version]:   # (as _mask_entry: never hit again)
            m = self._mask_cache.pop(old)[2]
            if m is not None:
                m.close()
        current = list(self._mask_cache.items())
        new_of_old = self._index.compact(carry=[e[2] for _, e in current if e[2] is not None] + self._resident_columns())
        keep = np.flatnonzero(new_of_old != np.uint64(0xFFFFFFFFFFFFFFFF))   # the old row of every new row, ascending
        n_old = len(self._id_of)
        self._id_of = [self._id_of[r] for r in keep]
        self._meta = [self._meta[r] for r in keep]
        self._row_of = {id_: i for i, id_ in enumerate(self._id_of)}
        self._version += 1
        self._mask_cache = {}
        for (key, _), (words, flt, mask) in current:
            if mask is not None:
                words = mask.read().reshape(1, -1)
            else:   # host words only: the same selection with numpy
                bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n_old]
                words = pack_allow_bits(bits[keep].astype(bool))
            self._mask_cache[(key, self._version)] = [words, flt, mask]
        self.compactions += 1
        return dropped

    def GetDocumentCount(self) -> int:
        return len(self._row_of)

    def GetAllIDs(self):
        return sorted(self._row_of)

    def computeAverageDistance(self, samples: int, intn=None) -> float:
        """collection.go:348-400: mean distance over up to `samples` random pairs of
        distinct documents.  `intn(n)` plays rand.Intn (Go's generator is the caller's);
        the pairs' distances come from one szg_pair_distances call, the in-order float64
        sum and the division stay here as in the reference (:389-398)."""
        if samples <= 0:
            return 0.0
        ids = self.GetAllIDs()
        if len(ids) < 2:
            return 0.0
        if intn is None:
            import random
            intn = random.randrange
        a, b = [], []
        for _ in range(samples):
            id1 = ids[intn(len(ids))]
            id2 = ids[intn(len(ids))]
            if id1 == id2:
                continue  # :375-377
            a.append(self._row_of[id1])
            b.append(self._row_of[id2])
        if not a:
            return 0.0
        total = 0.0
        for d in self._index.pair_distances(a, b):
            total += float(d)
        return total / float(len(a))

    def Close(self):
        if not self._closed:
            self._mask_cache.clear()
            self._index.close()   # (closes the masks it still holds first)
            self._closed = True

    # -- metadata fields resident on the card ------------------------------------
    def IndexField(self, name: str, kind: str):
        """Keep the top-level metadata field `name` as a column on the card (not in the reference): kind "number"
        holds the rows whose value is a JSON number; kinds "string" and "text" both hold those whose value is a string.
        "string" suits a field with few distinct values (a brand, a status): one 4-byte code per row of an append-only
        dictionary kept here, and a filter is evaluated on the host once per DISTINCT value.  "text" suits a field
        whose values are mostly distinct (an email, a name, an id): the strings' bytes live on the card, with no
        dictionary, and the card compares them (constants of up to 256 bytes, IN-lists of up to 16, and MATCHES
        patterns walked as a byte automaton).  The resident metadata is parsed once, now; from then on AddDocument(s) append to the column, UpdateDocument sets the row,
        and Compact() and the re-sort carry it along on the card.  Search with SearchArgs.Where then compares the field on the card."""
        if kind not in ("number", "string", "text"):
            raise ValueError('kind is "number", "string" or "text"')
        _where.Field(name)   # (the name must be an identifier of the filter language)
        old = self._fields.pop(name, None)
        if old is not None and old.column is not None:
            old.column.close()
        f = self._fields[name] = _FieldIndex(name, kind)
        parsed = [_where.parse_metadata(m) for m in self._meta]
        self._build_column(f, parsed)
        if self._object_col is None:
            self._object_col = self._index.column(np.array([d is not None for d in parsed], dtype=np.uint32),
                                                  kind=_lib.SZG_COL_U32)
        self._version += 1   # (cached Where masks that took the fallback for this field are re-made through the column)

    def _build_column(self, f, parsed):
        pairs = [f.value_of(d) for d in parsed]
        present = np.array([p for _, p in pairs], dtype=bool)
        if f.kind == "text":
            f.column = self._index.text_column([v for v, _ in pairs], present=present)
            return
        values = np.array([v for v, _ in pairs], dtype=np.float64 if f.kind == "number" else np.uint32)
        f.column = self._index.column(values, present=present,
                                      kind=_lib.SZG_COL_F64 if f.kind == "number" else _lib.SZG_COL_U32)

    def _resident_columns(self):
        """Every indexed field's column and the hidden object column: what a compaction or a re-sort carries.  (A
        "string" field's dictionary stays as it is: the codes are what travels.)"""
        if not self._fields:
            return []
        return [f.column for f in self._fields.values()] + [self._object_col]

    def _rebuild_columns(self):
        """Every column made again from the resident metadata (a json.loads per document, every column uploaded).
        Nothing in the package calls this today: Compact, auto_compact and the re-sort carry the columns on the card.
        It is kept as the way back for a path that would replace the rows without a list to carry by, and as the
        parent's route that scripts/dev_compact_columns.py times; column_rebuilds counts its calls."""
        self.column_rebuilds += 1
        if not self._fields:
            return
        parsed = [_where.parse_metadata(m) for m in self._meta]
        for f in self._fields.values():
            f.column.close()
            self._build_column(f, parsed)
        self._object_col.close()
        self._object_col = self._index.column(np.array([d is not None for d in parsed], dtype=np.uint32),
                                              kind=_lib.SZG_COL_U32)

    def _columns_append(self, n):
        """The last n rows are new: bring every column up to the index."""
        if not self._fields or n == 0:
            return
        parsed = [_where.parse_metadata(m) for m in self._meta[len(self._meta) - n:]]
        for f in self._fields.values():
            pairs = [f.value_of(d) for d in parsed]
            f.column.append([v for v, _ in pairs], present=np.array([p for _, p in pairs], dtype=bool))
        self._object_col.append(np.array([d is not None for d in parsed], dtype=np.uint32))

    def _columns_set(self, row):
        """Row `row`'s metadata changed."""
        if not self._fields:
            return
        data = _where.parse_metadata(self._meta[row])
        for f in self._fields.values():
            v, present = f.value_of(data)
            f.column.set(row, v if present else None)
        self._object_col.set(row, 1 if data is not None else 0)

    def _columns_set_rows(self, rows):
        """The metadata of `rows` (each listed once) changed: number and string fields, and the hidden object column,
        take their new values in one set_rows each; a text field's values go row by row."""
        if not self._fields or not rows:
            return
        parsed = [_where.parse_metadata(self._meta[row]) for row in rows]
        for f in self._fields.values():
            pairs = [f.value_of(d) for d in parsed]
            if f.kind == "text":
                for row, (v, present) in zip(rows, pairs):
                    f.column.set(row, v if present else None)
                continue
            f.column.set_rows(rows, [v for v, _ in pairs], present=np.array([p for _, p in pairs], dtype=bool))
        self._object_col.set_rows(rows, np.array([d is not None for d in parsed], dtype=np.uint32))

    def _leaf_mask(self, e):
        """(mask, can_error) of one leaf through its field's column: mask = the rows where the leaf is true AND the
        field holds a value of the indexed type.  None: the leaf cannot be answered by the columns (field not indexed,
        a constant of another type than the index, an IN-list beyond the kernel's) -- the caller falls back."""
        f = self._fields.get(e.field)
        if f is None:
            return None
        want = float if f.kind == "number" else str
        col = f.column
        if isinstance(e, _where.Matches):
            if f.kind == "string":   # once per dictionary entry, like a string operator
                return col.codes([e.test(s) for s in f.codes]), True
            if f.kind != "text":
                return None
            try:   # the pattern's whole table on the card; one beyond the kernel's limits: the host answers
                dfa = e.matcher.dfa()
            except _regex_dfa.DfaTooLarge:
                return None
            return col.dfa(dfa), True
        if f.kind == "text":
            return self._text_leaf_mask(e, col)
        if isinstance(e, _where.Cmp):
            if not isinstance(e.constant, want):
                return None
            positive = _where.Cmp(e.field, "==", e.constant) if e.op == "!=" else e
            if f.kind == "number":
                m = col.where(positive.op, positive.constant)
            else:
                m = col.codes([positive.test(s) for s in f.codes])
            if e.op == "!=":   # true for nil and every value of another type as well: the complement
                m, pos = ~m, m
                pos.close()
            return m, e.op in _where._ORDERED
        if isinstance(e, _where.In):
            if not all(isinstance(c, want) for c in e.constants) or len(e.constants) > 1024:
                return None
            if f.kind == "number":
                m = col.isin(e.constants)
            else:
                inside = set(e.constants)
                m = col.codes([s in inside for s in f.codes])
            if e.negate:
                m, pos = ~m, m
                pos.close()
            return m, False
        if isinstance(e, _where.StrOp):
            if f.kind != "string":
                return None
            return col.codes([e.test(s) for s in f.codes]), True
        return None

    @staticmethod
    def _text_leaf_mask(e, col):
        """_leaf_mask for a "text" field: the card compares the bytes.  None (the host answers) for a constant that is
        not a string or is longer than the kernel's 256 bytes, and for an IN-list of more than 16 strings."""
        def fits(c):
            return isinstance(c, str) and len(_where._bytes(c)) <= _lib.SZG_STR_PATTERN_MAX

        if isinstance(e, _where.Cmp):
            if not fits(e.constant):
                return None
            if e.op == "!=":   # true for nil and every value of another type as well: the complement of ==
                pos = col.where("==", e.constant)
                m = ~pos
                pos.close()
                return m, False
            return col.where(e.op, e.constant), e.op in _where._ORDERED
        if isinstance(e, _where.In):
            if not all(fits(c) for c in e.constants) or len(e.constants) > 16:
                return None
            m = None
            for c in dict.fromkeys(e.constants):   # the OR of the == masks
                eq = col.where("==", c)
                if m is None:
                    m = eq
                else:
                    m, old = m | eq, m
                    old.close()
                    eq.close()
            if m is None:   # an empty list: no row
                everyone = col.present()
                m = everyone.andnot(everyone)
                everyone.close()
            if e.negate:
                m, pos = ~m, m
                pos.close()
            return m, False
        if isinstance(e, _where.StrOp):
            if not fits(e.constant):
                return None
            fn = {"STARTS_WITH": col.startswith, "ENDS_WITH": col.endswith, "CONTAINS": col.contains}[e.op]
            return fn(e.constant), True
        return None

    def _where_device_mask(self, expr):
        """The expression as a ScanMask through the columns: V(expr) -- plain mask algebra over the leaves -- &
        "the metadata is a JSON object" & present(field) of every leaf that can error (where.py has the rules).
        None: some leaf needs the host (the masks made so far are closed)."""
        made, need = [], set()

        def V(e):
            if isinstance(e, (_where.And, _where.Or)):
                a = V(e.a)
                b = V(e.b) if a is not None else None
                if b is None:
                    return None
                m = (a & b) if isinstance(e, _where.And) else (a | b)
            elif isinstance(e, _where.Not):
                a = V(e.a)
                if a is None:
                    return None
                m = ~a
            else:
                leaf = self._leaf_mask(e)
                if leaf is None:
                    return None
                m, can_error = leaf
                if can_error:
                    need.add(e.field)
            made.append(m)
            return m

        try:
            v = V(expr)
            if v is None:
                return None
            guard = self._object_col.codes([False, True])
            made.append(guard)
            for name in sorted(need):
                guard = self._fields[name].column.present(base=guard)
                made.append(guard)
            result = v & guard
        finally:
            for m in made:   # (the temporaries; the result is a mask of its own)
                m.close()
        return result

    def _where_filter(self, expr):
        return lambda id_, meta: expr.evaluate(meta)

    def _where_handle(self, expr):
        """The Where expression's verdicts as a ScanMask, cached per (expr.text(), collection version) beside the
        Filter masks: compiled through the columns, or -- when a leaf cannot be -- evaluated on the host like a Filter
        with expr.text() as its key."""
        key = expr.text()
        hit = self._mask_cache.get((key, self._version))
        if hit is None and self._fields:
            self._drop_old_masks()
            mask = self._where_device_mask(expr)
            if mask is not None:
                self.where_compiled += 1
                if len(self._mask_cache) > 16:
                    self._mask_cache.clear()
                hit = self._mask_cache[(key, self._version)] = [mask.read().reshape(1, -1), self._where_filter(expr), mask]
        if hit is None:
            self.where_fallbacks += 1
        return self._allow_handle(self._where_filter(expr), key)

    def _search_filter(self, args):
        """(filter callable, cache key, where expression) of a Search: Filter and Where are exclusive."""
        expr = getattr(args, "Where", None)
        if expr is None:
            return args.Filter, getattr(args, "FilterKey", None), None
        if args.Filter is not None:
            raise ValueError("SearchArgs: Filter and Where are exclusive")
        if not isinstance(expr, _where.Expr):
            raise TypeError("SearchArgs.Where is a where.Expr")
        return self._where_filter(expr), expr.text(), expr

    def _search_handle(self, args):
        flt, key, expr = self._search_filter(args)
        return self._where_handle(expr) if expr is not None else self._allow_handle(flt, key)

    # -- Search ---------------------------------------------------------------
    def _drop_old_masks(self):
        # the version has moved: entries of older versions can never be hit again, their device masks go now
        for old in [k for k in self._mask_cache if k[1] != self._version]:
            m = self._mask_cache.pop(old)[2]
            if m is not None:
                m.close()

    def _allow_mask(self, flt, key=None):
        """One bit per row from the caller's filter (collection.go:592-594).  `key` (e.g. the
        REST layer's filter text) makes the verdicts reusable until the collection changes;
        without it the filter object itself is the key."""
        if flt is None:
            return None
        return self._mask_entry(flt, key)[0]

    def _mask_entry(self, flt, key):
        ck = (key if key is not None else id(flt), self._version)
        hit = self._mask_cache.get(ck)
        if hit is not None and (key is not None or hit[1] is flt):
            return hit
        self._drop_old_masks()
        mask = np.zeros(len(self._id_of), dtype=bool)
        for row, id_ in enumerate(self._id_of):
            if id_ is not None:
                mask[row] = bool(flt(id_, self._meta[row]))
        bits = pack_allow_bits(mask)
        if len(self._mask_cache) > 16:
            self._mask_cache.clear()   # (a mask a batch in the making still refers to lives on until that drops it)
        hit = self._mask_cache[ck] = [bits, flt, None]
        return hit

    def _allow_handle(self, flt, key=None):
        """The filter's verdicts as a ScanMask on the card, made once per (filter key, collection version)."""
        if flt is None:
            return None
        hit = self._mask_entry(flt, key)
        if hit[2] is None:
            hit[2] = self._index.mask(hit[0])
        return hit[2]

    def Search(self, args: SearchArgs) -> SearchResults:
        """collection.go:569-711."""
        n_records = len(self._row_of)
        results: List[SearchResult] = []
        points_searched = 0

        flt = self._search_filter(args)[0]
        if args.Radius == 0 and args.K == 0:
            # listing mode (collection.go:633-669): sorted *string* id order
            for id in sorted(self._row_of, key=lambda i: str(i)):
                row = self._row_of[id]
                if flt is not None and not flt(id, self._meta[row]):
                    continue
                points_searched += 1
                if args.Offset > 0 and points_searched <= args.Offset:
                    continue
                results.append(SearchResult(ID=id, Metadata=self._meta[row]))
                if args.Limit > 0 and len(results) >= args.Limit:
                    break
        else:
            q = np.asarray(args.Vector, dtype=np.float64).reshape(-1)
            if q.size != self.DimensionCount:
                # undefined in the reference (collection.go:814, :823); rejected here
                raise ValueError("query length %d != dimension %d" % (q.size, self.DimensionCount))

            def scan():
                if n_records == 0:
                    return [], []
                mask = self._search_handle(args)
                if args.Radius > 0:  # K is ignored (collection.go:598-605)
                    return self._index.search_radius(q, args.Radius, masks=mask)
                r, d, c = self._index.search_topk(q, args.K, masks=mask)
                return r[0, : c[0]], d[0, : c[0]]
            if self._order_stale and self._index.options.get("tie_mode", 0) != 0:
                # tie_mode 1 keeps the fast answer for ties and counts no replay: the test below would never see one,
                # so the deterministic mode re-pages up front
                self._resort()
            if self._order_stale:
                # rows out of sort.Strings order: did the answer depend on the visit order?  (the library re-answers
                # ties among the best k+1 by an exact replay in ROW order and counts it; a radius result depends on
                # the order when two of its distances are equal)
                before = self._index.stats()["full_replays"]
                rows, dist = scan()
                tie = self._index.stats()["full_replays"] != before or \
                    (args.Radius > 0 and len(set(float(x) for x in dist)) != len(dist))
                if tie:
                    self._resort()
                    rows, dist = scan()
            else:
                rows, dist = scan()
            for row, dd in zip(rows, dist):
                row = int(row)
                results.append(SearchResult(ID=self._id_of[row], Metadata=self._meta[row],
                                            Distance=float(dd)))
            points_searched = n_records  # counted before the filter (collection.go:589)

        percent = float(points_searched) / float(n_records) * 100 if n_records else 0.0
        return SearchResults(Results=results, PercentSearched=percent)

    def SearchBatch(self, args_list) -> List[SearchResults]:
        """Exact Searches of a caller that holds many queries (not in the reference, whose REST endpoint is
        single-query, rest.go:371-487): top-k Searches with one K share ONE szg_search_topk call -- and with it
        sweeps on the matrix cores --, radius Searches one szg_search_radius_batch; each query keeps its own
        Filter.  Anything else (listing mode, mixed kinds) is answered Search by Search.  Same results as Search."""
        args_list = list(args_list)
        n_records = len(self._row_of)
        if not args_list:
            return []
        radius = args_list[0].Radius > 0
        same = all((a.Radius > 0) == radius and (radius or (a.K == args_list[0].K and a.K > 0)) for a in args_list)
        if not same or n_records == 0:
            return [self.Search(a) for a in args_list]
        if self._order_stale:
            self._resort()   # (a batch is not worth the tie bookkeeping: deterministic mode re-pages first)
        Q = np.stack([np.asarray(a.Vector, dtype=np.float64).reshape(-1) for a in args_list])
        if Q.shape[1] != self.DimensionCount:
            raise ValueError("query length %d != dimension %d" % (Q.shape[1], self.DimensionCount))
        masks = None
        if any(a.Filter is not None or getattr(a, "Where", None) is not None for a in args_list):
            # one handle per query (None = unfiltered); queries that share a FilterKey share the handle, and a batch
            # that holds a single one passes just that: its sweeps read the resident mask in place
            masks = [self._search_handle(a) for a in args_list]
            if all(m is masks[0] for m in masks):
                masks = masks[0]
        out = []
        if radius:
            hits = self._index.search_radius_batch(Q, [a.Radius for a in args_list], masks=masks)
        else:
            r, d, c = self._index.search_topk(Q, args_list[0].K, masks=masks)
            hits = [(r[i, : c[i]], d[i, : c[i]]) for i in range(len(args_list))]
        for rows, dist in hits:
            res = [SearchResult(ID=self._id_of[int(row)], Metadata=self._meta[int(row)], Distance=float(dd))
                   for row, dd in zip(rows, dist)]
            out.append(SearchResults(Results=res, PercentSearched=100.0))
        return out

    def SearchBatchTensor(self, queries, K=0, Radius=0.0, Filter=None, Where=None, FilterKey=None) -> List[SearchResults]:
        """SearchBatch for queries that lie in device memory (not in the reference): row i of the 2-D device tensor
        `queries` (ScanIndex.search_topk_tensor) is query i, all with one K -- or one Radius, which as ever wins over K
        -- and ONE filter for the whole batch.  The results are SearchBatch's for the same vectors widened to float64
        on the host, PercentSearched included.  Listing mode (K == 0 and Radius == 0) has no vector and is refused."""
        shape = tuple(queries.shape)
        if len(shape) != 2 or shape[1] != self.DimensionCount:
            raise ValueError("query length does not match the dimension %d: shape %r" % (self.DimensionCount, shape))
        if not (Radius > 0 or K > 0):
            raise ValueError("SearchBatchTensor: K > 0 or Radius > 0 (listing mode takes no vectors: Search)")
        args = SearchArgs(K=K, Radius=Radius, Filter=Filter, Where=Where, FilterKey=FilterKey)
        flt = self._search_filter(args)[0]  # (Filter and Where are exclusive: said before anything is searched)
        n_records = len(self._row_of)
        if n_records == 0:
            return [SearchResults(Results=[], PercentSearched=0.0) for _ in range(shape[0])]
        if self._order_stale:
            self._resort()   # (as SearchBatch: deterministic mode re-pages first)
        mask = self._search_handle(args) if (flt is not None or Where is not None) else None
        if Radius > 0:
            hits = self._index.search_radius_tensor(queries, Radius, masks=mask)
        else:
            r, d, c = self._index.search_topk_tensor(queries, K, masks=mask)
            hits = [(r[i, : c[i]], d[i, : c[i]]) for i in range(shape[0])]
        out = []
        for rows, dist in hits:
            res = [SearchResult(ID=self._id_of[int(row)], Metadata=self._meta[int(row)], Distance=float(dd))
                   for row, dd in zip(rows, dist)]
            out.append(SearchResults(Results=res, PercentSearched=100.0))
        return out
