/*
 * syzgy_scan.h -- C ABI of the MI355X-native brute-force scan that drops in
 * behind SyzgyDB's Collection.Search (Precision "exact").
 *
 * The reference (smhanov/syzgydb, Go) has no FFI seam today; the seam this
 * library replaces is the block
 *     collection.go:672-684   (IterateRecords + consider(), the HOT LOOP)
 * together with the per-record work it calls:
 *     collection.go:583-629   consider(): filter, distance, top-k / radius
 *     collection.go:768-794   decodeVector     quantization.go:25-36 dequantize
 *     collection.go:812-832   euclideanDistance / angularDistance
 *     collection.go:536-564   resultPriorityQueue (container/heap)
 * The Go side keeps SearchArgs / SearchResults / SearchResult
 * (collection.go:115-158) unchanged; go/syzgy_gpu.go shows the cgo binding and
 * INTEGRATION.md the edit to Collection.Search.
 *
 * Conventions: extern "C", plain pointers and explicit sizes, no exceptions
 * cross the boundary.  Every function returns SZG_OK (0) or a negative
 * SZG_E_* code.  All in/out buffers are caller-owned and only borrowed for the
 * duration of the call (cgo rule: no Go pointer is retained).  A handle may
 * be used by any number of threads concurrently for szg_search_* (the
 * reference runs Searches concurrently under RLock, collection.go:570);
 * load/append/tombstone/overwrite need exclusive access (the reference's
 * write lock, collection.go:428, :512).
 *
 * Rows are addressed by their position in the VISIT ORDER the caller loaded
 * them in (spanfile.go:521-560); the caller keeps the row -> document-id table.
 */
#ifndef SYZGY_SCAN_H
#define SYZGY_SCAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SZG_ABI_VERSION 4

/* DistanceMethod, collection.go:186-189 */
#define SZG_EUCLIDEAN 0
#define SZG_COSINE 1

#define SZG_OK 0
#define SZG_E_INVALID (-1)    /* bad argument (dim, quantization, metric, k, null pointer) */
#define SZG_E_NOMEM (-2)      /* host or device allocation failed */
#define SZG_E_DEVICE (-3)     /* HIP runtime error; szg_last_error() has the text */
#define SZG_E_TRUNCATED (-4)  /* radius search: more hits than `capacity`; *out_total says how many */
#define SZG_E_NODEVICE (-5)   /* no usable gfx950 device / HIP kernels not loadable */
#define SZG_E_RANGE (-6)      /* row index out of range */
#define SZG_E_UNSUPPORTED (-7)/* valid in the reference but outside this build's limits */

typedef struct szg_index szg_index;

/*
 * One handle per Collection (created where NewCollection pages the corpus,
 * collection.go:297-311; destroyed in Collection.Close, :408-421).
 *   dim         CollectionOptions.DimensionCount
 *   quant_bits  CollectionOptions.Quantization: 4, 8, 16, 32 or 64 (collection.go:796-811)
 *   metric      SZG_EUCLIDEAN or SZG_COSINE (collection.go:275-283)
 *   devices     HIP device ordinals to shard the rows over (contiguous row
 *               ranges, one per entry); NULL / n_devices==0 = current device.
 */
int szg_index_create(szg_index **out, int dim, int quant_bits, int metric,
                     const int *devices, int n_devices);
void szg_index_destroy(szg_index *ix);

/* Row byte size = getVectorSize(quant_bits, dim), collection.go:796-811; <0 on error. */
int64_t szg_row_bytes(int quant_bits, int dim);

/*
 * Replace the mirror's content with n_rows packed vectors in the reference's
 * on-disk element encoding (stream 1 of each span: 4-bit high-nibble-first,
 * 8-bit bytes, big-endian 16/32/64-bit; collection.go:713-743).  Copies.
 */
int szg_index_load(szg_index *ix, const uint8_t *rows, uint64_t n_rows);

/* AddDocument (collection.go:427-457): rows go to the end of the visit order. */
int szg_index_append(szg_index *ix, const uint8_t *rows, uint64_t n_rows);

/*
 * AddDocument for a block of float64 vectors (bulk ingest): quantize + pack on the
 * device exactly as encodeDocument / quantize do (collection.go:713-743,
 * quantization.go:5-23), rows go to the end of the visit order.
 */
int szg_index_append_f64(szg_index *ix, const double *vectors, uint64_t n_rows);

/* AddDocument on an existing id rewrites the record: replace one row in place
 * (from packed bytes, or from a float64 vector encoded on the device). */
int szg_index_overwrite_f64(szg_index *ix, uint64_t row, const double *vector);
int szg_index_overwrite(szg_index *ix, uint64_t row, const uint8_t *row_bytes);

/* removeDocument (collection.go:511-521): the row is skipped by every later scan. */
int szg_index_tombstone(szg_index *ix, uint64_t row);

/* rows loaded (tombstoned ones included) / rows still live */
uint64_t szg_index_rows(const szg_index *ix);
uint64_t szg_index_live_rows(const szg_index *ix);

/* Read rows back in the reference encoding (inverse of the page-in transform). */
int szg_index_read_rows(szg_index *ix, uint64_t first_row, uint64_t n_rows, uint8_t *out);

/*
 * Exact top-k, i.e. Search{Precision:"exact", K:k, Radius:0}
 * (collection.go:606-619, :672-684, :694-697) for n_queries independent
 * queries.
 *   queries     n_queries x dim float64, SearchArgs.Vector (never quantized)
 *   allow_bits  NULL, or n_queries(!) x ceil(rows/64) words: bit r of query
 *               q's mask = args.Filter(id(r), metadata(r)) (collection.go:592)
 *   out_rows    n_queries x k row indices, ascending distance (:694-697)
 *   out_dist    n_queries x k float64 distances, the reference's own values
 *   out_count   n_queries result counts (<= k; fewer when fewer rows qualify)
 * Unused tail entries of out_rows are UINT64_MAX.
 */
int szg_search_topk(szg_index *ix, const double *queries, int n_queries, int k,
                    const uint64_t *allow_bits, uint64_t *out_rows, double *out_dist,
                    int32_t *out_count);

/*
 * Radius search, i.e. Search{Precision:"exact", Radius:radius>0} (K ignored,
 * collection.go:598-605).  Writes the min(total, capacity) closest hits in
 * ascending distance; *out_total is the full hit count.  Returns
 * SZG_E_TRUNCATED when total > capacity (retry with a larger buffer).
 */
int szg_search_radius(szg_index *ix, const double *query, double radius,
                      const uint64_t *allow_bits, uint64_t *out_rows, double *out_dist,
                      uint64_t capacity, uint64_t *out_total);

/*
 * Radius searches for a batch of queries, each with its own radius: the collect sweeps of the batch are walked
 * query-major by one launch per 16 queries, several launches in flight (collection.go:598-605 per query).
 *   allow_bits   NULL, or n_queries x ceil(rows/64) words
 *   out_offsets  n_queries + 1 entries: the hits of query i are out_rows / out_dist [out_offsets[i], out_offsets[i+1]),
 *                ascending distance
 * When the hits do not fit `capacity` the call returns SZG_E_TRUNCATED with out_offsets complete (so
 * out_offsets[n_queries] is the capacity to retry with) and the first `capacity` entries written.
 */
int szg_search_radius_batch(szg_index *ix, const double *queries, int n_queries, const double *radii,
                            const uint64_t *allow_bits, uint64_t *out_rows, double *out_dist, uint64_t capacity,
                            uint64_t *out_offsets);

/* ---- device-resident filter masks (added under ABI 4, additive) -------------
 *
 * args.Filter's verdicts (collection.go:592-594) as an object on the card: the host creates a mask once per
 * (filter, collection version) -- from words, from a row list, or composed on the device from other masks with the
 * operators of the reference's filter language -- and searches take the handle instead of uploading
 * n_queries x ceil(rows/64) words with every call.
 *
 * Same answers as allow_bits: a masked search returns what szg_search_topk / szg_search_radius_batch return when
 *   given szg_mask_read's words -- ids, float64 distances and order -- on every path: one sweep per query (dense and
 *   selective form), shared sweeps, radius batches, the sketch pre-pass, escalation, the full replay under tie_mode 0
 *   and handles whose shards share a process.
 * Tail bits: bits at positions >= rows are stored as 0, after SZG_MASK_NOT as well; szg_mask_count never counts them.
 * Mutations: szg_index_tombstone and the overwrites leave a mask valid (tombstones are applied through the live
 *   bits, as ever).  szg_index_load, szg_index_synth and the appends -- which change the row count -- make every
 *   older mask of the handle STALE: a search or combine with a stale mask returns SZG_E_INVALID ("stale mask" in
 *   szg_last_error) and never reads past the mask; so does a mask of another handle.  Stale masks can still be read,
 *   counted and destroyed.  szg_index_compact / szg_index_reorder rewrite the masks they are asked to carry and make
 *   the others stale.
 * Lifetime and threads: masks are destroyed before their handle.  Any number of threads may search with one mask
 *   concurrently; create / combine / destroy may run beside searches that do not use that mask.
 * Coalescing: szg_search_topk_masked with ONE query goes through the combiner like szg_search_topk; callers that all
 *   hold the same handle form a batch that reads the resident mask in place.  A coalesced batch that mixes raw-word
 *   callers and handle callers is staged through the host path, with the handles' host copy of the words.
 * Out of scope: szg_search_*_sharded keep allow_bits only.
 */
typedef struct szg_mask szg_mask;
#define SZG_MASK_AND 0      /* a & b */
#define SZG_MASK_OR 1       /* a | b */
#define SZG_MASK_ANDNOT 2   /* a & ~b */
#define SZG_MASK_NOT 3      /* ~a, b must be NULL */

/* bit r = row r may be visited; ceil(rows/64) words, copied. */
int szg_mask_create(szg_index *ix, const uint64_t *allow_bits, szg_mask **out);
/* exactly the listed rows (numbered as searches return them: local + row base); duplicates allowed;
   a row >= rows -> SZG_E_RANGE; n_rows == 0 -> the empty mask */
int szg_mask_create_rows(szg_index *ix, const uint64_t *rows, uint64_t n_rows, szg_mask **out);
/* composed on the device; a and b belong to the same handle and the same row count */
int szg_mask_combine(int op, const szg_mask *a, const szg_mask *b, szg_mask **out);
uint64_t szg_mask_count(const szg_mask *m);            /* rows allowed, exact */
int szg_mask_read(const szg_mask *m, uint64_t *out_bits); /* ceil(rows/64) words */
void szg_mask_destroy(szg_mask *m);                    /* NULL is fine */

/* n_masks == 1: masks[0] filters every query; n_masks == n_queries: one per query, NULL entry = unfiltered;
   masks == NULL / n_masks == 0: unfiltered.  Everything else as szg_search_topk / szg_search_radius_batch. */
int szg_search_topk_masked(szg_index *ix, const double *queries, int n_queries, int k,
                           const szg_mask *const *masks, int n_masks,
                           uint64_t *out_rows, double *out_dist, int32_t *out_count);
int szg_search_radius_masked(szg_index *ix, const double *queries, int n_queries, const double *radii,
                             const szg_mask *const *masks, int n_masks,
                             uint64_t *out_rows, double *out_dist, uint64_t capacity, uint64_t *out_offsets);

typedef struct szg_mask_stats {
    uint64_t live_masks, device_bytes;  /* masks alive on this handle, their device memory */
    uint64_t h2d_bytes;       /* filter words searches uploaded from host memory (the allow_bits path) */
    uint64_t d2d_bytes;       /* filter words copied card-to-card into a batch's per-query slots */
    uint64_t shared_batches;  /* batches whose sweeps read ONE resident mask in place (no copy at all) */
} szg_mask_stats;
int szg_index_mask_stats(szg_index *ix, szg_mask_stats *out);   /* szg_reset_stats clears the three counters */

/* ---- compaction and reorder on the device (added under ABI 4, additive) ------
 *
 * A tombstoned row keeps its bytes in device memory, is still read by every sweep, and its mere presence makes every
 * launch of its shard a masked one (no grouped 8-bit sweep, no unmasked launch geometry) -- unless sketch_masked = 1, under
 * which the sketch pre-pass's launches keep the matrix sweep.  These two calls renumber
 * the resident rows without a trip through the host: one gather kernel copies the kept rows, 16 bytes per lane, into
 * a NEW allocation sized for them, then the old one is freed -- so compaction gives device memory back, and the peak
 * during the call is the old plus the new allocation (per shard).
 *
 * Both need exclusive access, like every mutation, and synchronise the handle's devices first.  Afterwards the handle
 * is what a fresh one is after szg_index_load of the same rows in the same order: szg_index_rows ==
 * szg_index_live_rows, no tombstones, shard ranges and capacities as a load gives them (appends go on working), row
 * norms and the sketch rebuilt on the device by the next search that wants them.
 * Masks: carry[0 .. n_carry) are masks of this handle that are not stale; their words are rewritten for the new
 *   numbering on the device in the same call (new bit i = old bit of the row that became row i), count and
 *   szg_mask_read follow, and they STAY VALID.  Every other mask of the handle becomes stale, as after
 *   szg_index_load.  A null, foreign or stale entry in carry is SZG_E_INVALID.
 * Failure: every check happens on the host before anything moves, and any error -- bad arguments, SZG_E_NOMEM from
 *   the new allocation, a refused mask -- leaves rows, live bits, masks and the sketch exactly as they were.
 * Handles of several shards move rows between devices through the shards' staging buffers, at most 64 MiB at a time:
 *   two passes over the rows instead of one, at a cost that does not depend on how the list interleaves the shards.
 *   The internal sketch index of a float32 (or float64) handle is dropped with the old rows (its memory is returned too) and built
 *   again by the next search that wants it.  Sharded-search communicators are unaffected.
 */

/* New row i = old row src_rows[i] (rows numbered as searches return them: local + row base); rows not listed are
 * dropped.  Every listed row must be in range (else SZG_E_RANGE), live and listed once (else SZG_E_INVALID).
 * n_rows == 0 empties the index. */
int szg_index_reorder(szg_index *ix, const uint64_t *src_rows, uint64_t n_rows,
                      szg_mask *const *carry, int n_carry);

/* Drop the tombstoned rows, keeping the order of the live ones (the reference's visit order).
 * out_new_of_old: nullable, szg_index_rows() entries before the call: the new number of each old row (+ row base),
 * UINT64_MAX for a dropped one.  *out_rows (nullable) = rows afterwards.  No tombstones: returns SZG_OK, moves
 * nothing, and no mask becomes stale. */
int szg_index_compact(szg_index *ix, uint64_t *out_new_of_old, uint64_t *out_rows,
                      szg_mask *const *carry, int n_carry);

/* ---- resident metadata columns (added under ABI 4, additive) -----------------
 *
 * The leaves of the reference's filter language on the card.  A top-level metadata field becomes a column resident
 * beside the rows -- one value and one present bit per row -- and a comparison against a constant is ONE
 * bandwidth-bound kernel per shard that writes the words and the count of an ordinary szg_mask.  A new filter text
 * (`price < 37.5`) then costs a few small launches and never walks the per-row metadata on the host; the masks compose
 * with szg_mask_combine like any others.
 *
 * Kinds: SZG_COL_F64 holds doubles; SZG_COL_U32 holds codes of a dictionary the HOST owns (the library never sees the
 *   strings: the host evaluates a string operator once per dictionary entry into a bitmap over codes) -- the kind for
 *   a string field with few distinct values; SZG_COL_STR holds the strings themselves, for a field whose values are
 *   mostly distinct (see "Text columns" below).
 * Predicate of every szg_mask_where_*: bit r = present(r) && pred(value[r]) (&& base's bit r).  Float64 comparisons
 *   follow IEEE, i.e. Go's == and < on float64 (query/compiler.go:175, :288-303): -0.0 == 0.0, and a NaN fails every
 *   operator but SZG_CMP_NE.  Tail bits are 0, as in every mask.
 * Create and append: a column belongs to one handle and covers its rows [0, n): n_rows <= szg_index_rows(ix), else
 *   SZG_E_RANGE -- it may be shorter, so the host can append rows to the index first and bring the column up
 *   afterwards.  present_bits == NULL: every row is present; otherwise bit i = the i-th row OF THE CALL (for an append,
 *   the i-th appended row: the library shifts the bits into place, no alignment is asked of the caller).  Values and
 *   bits are copied.  An append past szg_index_rows returns SZG_E_RANGE.  Capacity grows geometrically.
 * Rows are numbered as searches return them (local + row base) in szg_column_set and szg_column_read.
 * Storage: each shard's part lives on the shard's device -- 8 or 4 bytes per row plus one bit -- next to a host copy
 *   of the present words.
 * szg_mask_where_*: need szg_column_rows(c) == szg_index_rows(owner), else SZG_E_INVALID ("short column" in
 *   szg_last_error).  base is nullable; when given it must be a mask of the same handle that is not stale (else
 *   SZG_E_INVALID), and the result is base & pred.  The result is an ordinary szg_mask in every respect: count, read,
 *   combine, searches, carry across compaction, szg_index_mask_stats; its host copy of the words is downloaded once,
 *   at creation.  An operator outside SZG_CMP_EQ..SZG_CMP_GE, or a column whose kind does not match the call, is
 *   SZG_E_INVALID.
 * Mutations: szg_index_tombstone and the overwrites leave a column valid; the appends leave it valid but short.
 *   szg_index_load, szg_index_synth, szg_index_reorder and a szg_index_compact that moves rows (one without
 *   tombstones does not) make it STALE: every call except szg_column_rows, szg_column_read and szg_column_destroy
 *   then returns SZG_E_INVALID ("stale column") and never reads past the column.  szg_index_reorder_carry and
 *   szg_index_compact_carry take the columns they are given along on the device, and those stay valid (see "Columns
 *   carried across compaction and reorder" below); a column they are not given goes stale all the same.
 * Threads: szg_mask_where_* and szg_column_read may run beside searches and beside each other; create / append / set /
 *   destroy need the exclusive access mutations have.  Columns are destroyed before their handle.
 * Failure: every check happens on the host before anything is allocated or launched; an error leaves the column as
 *   it was and *out untouched.
 * Text columns (SZG_COL_STR): values are BYTES, not text -- embedded NUL bytes and bytes >= 0x80 are ordinary -- and
 *   the card compares them as Go compares strings (query/compiler.go:304-319; strings.Contains / HasPrefix /
 *   HasSuffix, :393-418): unsigned, lexicographic, a proper prefix being the smaller.  They have calls of their own
 *   (szg_column_create_str / _append_str / _set_str / _read_str, szg_mask_where_str); szg_column_create keeps refusing
 *   the kind, and szg_column_append, szg_column_set, szg_column_read with out_values != NULL and
 *   szg_mask_where_f64 / _in_f64 / _u32 on a text column -- like szg_mask_where_str and the *_str calls on another
 *   kind -- return SZG_E_INVALID ("kind does not match").  szg_column_rows, szg_column_read with out_values == NULL,
 *   szg_mask_where_present and szg_column_destroy work on every kind.  Everything above -- row numbering, short and
 *   stale columns, base, threads, failure -- holds for them unchanged.
 *   Storage per shard part: one 8-byte reference {uint32 start, uint32 len} per row into the part's byte heap, the
 *   heap, and the present bits.  Create and append write a call's strings back to back in row order; an absent row
 *   has length 0.  The heap grows geometrically; its capacity is a multiple of 16 bytes that ends at least 16 zero
 *   bytes past the last used byte, and stays below 4 GiB per part: a call that would exceed that returns
 *   SZG_E_UNSUPPORTED with the column unchanged.  Dead bytes (szg_column_set_str) are reclaimed by a carry across a
 *   compaction or reorder, which repacks the heap, or by making the column again.
 *   szg_mask_where_str: op is SZG_CMP_EQ..SZG_CMP_GE or SZG_STR_STARTS_WITH / ENDS_WITH / CONTAINS, anything else
 *   SZG_E_INVALID ("operator" in szg_last_error); a constant of more than SZG_STR_PATTERN_MAX bytes is
 *   SZG_E_UNSUPPORTED, a NULL constant with len > 0 SZG_E_INVALID.  The empty constant is legal: the three string
 *   operators then hold for every present row, the comparisons run against "".  One kernel per shard, a lane per
 *   row: a match lies wholly inside its row.
 * Byte automata (szg_mask_where_dfa, text columns): bit r = present(r) && accept[the state after feeding ALL bytes of
 *   row r, in order, from `start`] (&& base's bit r); a row of length 0 gives accept[start].  The library knows nothing
 *   of regular expressions: the caller compiles its pattern language -- anchors, "match anywhere" and all -- into the
 *   table (syzgydb_amd/regex_dfa.py does so for the reference's MATCHES operator, query/compiler.go:420-431).  A byte b
 *   takes state s to next[s * n_classes + class_of[b]]; bit s of accept_bits says whether s accepts.  The tables are
 *   copied; everything said above of szg_mask_where_* holds unchanged.  Refusals, all before anything is allocated or
 *   launched: a NULL dfa or a NULL array is SZG_E_INVALID; n_states or n_classes of 0, n_classes > 256, a start, a
 *   class_of entry or a next entry out of range are SZG_E_INVALID with "dfa" in szg_last_error -- the table is checked
 *   in full, the kernel never indexes past it; n_states > SZG_DFA_STATES_MAX or n_states * n_classes >
 *   SZG_DFA_TABLE_MAX is SZG_E_UNSUPPORTED.  A state whose every transition is to itself is ABSORBING: the library
 *   finds these, and a lane that reaches one stops reading its row ("already matched", "can no longer match") -- what
 *   makes an unanchored pattern cheap on long rows.  One kernel per shard, a lane per row.
 */
typedef struct szg_column szg_column;
#define SZG_COL_F64 0   /* values: double */
#define SZG_COL_U32 1   /* values: uint32_t codes; the host owns the dictionary */
#define SZG_COL_STR 2   /* values: byte strings, resident beside the rows */
#define SZG_CMP_EQ 0
#define SZG_CMP_NE 1
#define SZG_CMP_LT 2
#define SZG_CMP_LE 3
#define SZG_CMP_GT 4
#define SZG_CMP_GE 5
#define SZG_STR_STARTS_WITH 6   /* szg_mask_where_str only: continue SZG_CMP_EQ..SZG_CMP_GE */
#define SZG_STR_ENDS_WITH 7
#define SZG_STR_CONTAINS 8
#define SZG_STR_PATTERN_MAX 256 /* bytes of a constant */
#define SZG_DFA_STATES_MAX 32768u        /* states are uint16; the library keeps bit 15 of a staged entry for itself */
#define SZG_DFA_TABLE_MAX  (1u << 20)    /* n_states * n_classes entries */
typedef struct szg_dfa {
    uint32_t n_states;            /* 1 .. SZG_DFA_STATES_MAX */
    uint32_t n_classes;           /* 1 .. 256 */
    uint32_t start;               /* < n_states */
    const uint8_t  *class_of;     /* 256 entries, each < n_classes: the byte's column in `next` */
    const uint16_t *next;         /* n_states * n_classes, row-major by state, each < n_states */
    const uint64_t *accept_bits;  /* ceil(n_states / 64) words */
} szg_dfa;

int szg_column_create(szg_index *ix, int kind, const void *values, const uint64_t *present_bits,
                      uint64_t n_rows, szg_column **out);
int szg_column_append(szg_column *c, const void *values, const uint64_t *present_bits, uint64_t n_rows);
/* one row: its value and present bit; value == NULL marks the row absent (its stored value stays) */
int szg_column_set(szg_column *c, uint64_t row, const void *value);
uint64_t szg_column_rows(const szg_column *c);
/* rows [first_row, first_row + n_rows) of the column: n_rows values and ceil(n_rows/64) words, bit i = row
   first_row + i, tail bits 0; either output may be NULL; past szg_column_rows -> SZG_E_RANGE.  Works on a stale column */
int szg_column_read(const szg_column *c, uint64_t first_row, uint64_t n_rows, void *out_values,
                    uint64_t *out_present_bits);
void szg_column_destroy(szg_column *c);   /* NULL is fine; before its handle */

/* text columns.  offsets: n_rows + 1 entries, offsets[0] == 0, non-decreasing (else SZG_E_INVALID, "offsets" in
   szg_last_error); row i of the call = bytes[offsets[i] .. offsets[i + 1]).  present_bits as szg_column_create */
int szg_column_create_str(szg_index *ix, const uint8_t *bytes, const uint64_t *offsets,
                          const uint64_t *present_bits, uint64_t n_rows, szg_column **out);
int szg_column_append_str(szg_column *c, const uint8_t *bytes, const uint64_t *offsets,
                          const uint64_t *present_bits, uint64_t n_rows);
/* one row: value == NULL marks the row absent (its bytes stay).  len <= the stored len: rewritten in place.  Longer:
   the bytes go to the end of the heap and the row points there; the old bytes are dead until the column is made again */
int szg_column_set_str(szg_column *c, uint64_t row, const uint8_t *value, uint64_t len);
/* rows [first_row, first_row + n_rows): out_offsets (nullable) gets n_rows + 1 entries, row i = out_bytes[out_offsets[i]
   .. out_offsets[i + 1]); out_bytes is nullable; capacity < out_offsets[n_rows] -> SZG_E_TRUNCATED with the offsets
   still valid.  Present words as szg_column_read.  Works on a stale column.  A test and debug path: it downloads the
   parts' references and heaps */
int szg_column_read_str(const szg_column *c, uint64_t first_row, uint64_t n_rows, uint64_t *out_offsets,
                        uint8_t *out_bytes, uint64_t capacity, uint64_t *out_present_bits);

/* present && value op constant (SZG_CMP_*) */
int szg_mask_where_f64(const szg_column *c, int op, double value, const szg_mask *base, szg_mask **out);
/* present && value == one of values[0 .. n_values): duplicates allowed, a NaN among them matches nothing, n_values == 0
   gives the empty mask; more than 1024 -> SZG_E_UNSUPPORTED */
int szg_mask_where_in_f64(const szg_column *c, const double *values, uint32_t n_values,
                          const szg_mask *base, szg_mask **out);
/* present && bit `code` of code_bits (n_codes bits, ceil(n_codes/64) words, copied); a code >= n_codes fails */
int szg_mask_where_u32(const szg_column *c, const uint64_t *code_bits, uint32_t n_codes,
                       const szg_mask *base, szg_mask **out);
/* text columns: present && value op constant[0 .. len), op SZG_CMP_* or SZG_STR_* */
int szg_mask_where_str(const szg_column *c, int op, const uint8_t *constant, uint32_t len,
                       const szg_mask *base, szg_mask **out);
/* text columns: present && the automaton accepts the row's bytes (see "Byte automata" above) */
int szg_mask_where_dfa(const szg_column *c, const szg_dfa *dfa, const szg_mask *base, szg_mask **out);
/* the present bits (every kind) */
int szg_mask_where_present(const szg_column *c, const szg_mask *base, szg_mask **out);

/* ---- columns carried across compaction and reorder (added under ABI 4, additive) ----
 *
 * szg_index_reorder and szg_index_compact with columns to take along: everything said of those two calls holds, and
 * they ARE these calls with n_columns == 0 (every column of the handle then goes stale).
 * Columns: columns[0 .. n_columns) are columns of this handle that are neither stale nor short; a duplicate is taken
 *   once.  Same reads: after the call a carried column reads at new row i exactly what it read at the old row that
 *   became row i -- through szg_column_read and szg_column_read_str alike: the value bit for bit (NaN payloads and
 *   -0.0 included), the present bit, and for a row marked absent its stored value or stored bytes too.  State
 *   afterwards: szg_column_rows == the new row count, the column is valid, its parts follow the new shard ranges, and
 *   capacities, present words (tail bits 0) and the heap's sizing are those of a freshly created column of these rows;
 *   szg_column_append, szg_column_set, the _str calls and every szg_mask_where_* go on working.  Every column NOT in
 *   the list becomes stale, as before.
 * Text columns: afterwards the heap of each part holds each carried row's bytes exactly once, back to back, and nothing
 *   else: szg_column_info.heap_used == the sum of the carried rows' lengths, the bytes behind it are zero, and the
 *   capacity is that of a fresh column of these bytes.  Dead bytes (szg_column_set_str) and the bytes of dropped rows
 *   are reclaimed.  The order of the bytes inside a part is not specified.  A destination part whose carried bytes
 *   would reach the 4 GiB heap limit returns SZG_E_UNSUPPORTED.
 * Refusals: a null entry, a column of another handle, a stale column ("stale column") and a short one ("short column",
 *   szg_column_rows != szg_index_rows) are SZG_E_INVALID.
 * szg_index_compact_carry on a handle without tombstones moves nothing, makes nothing stale and leaves heaps as they
 *   are.
 * Failure: every check and every allocation -- a text part's byte total, which comes from a scan on the device and is
 *   read back, included -- happens before the switch.  On any error the rows, live bits, masks and ALL columns, carried
 *   or not, are exactly as they were, and still valid.
 * Memory: the peak during the call is the old plus the new column allocations, beside what the rows take; a handle of
 *   one shard adds 24 bytes per row of scratch while a text column is repacked (the list, which rows and columns share,
 *   the gathered references and the new starts), a handle of several 16 bytes per row of a destination part for the
 *   lists, 16 more per row of a text column, and four staging buffers of at most 64 MiB.
 */
int szg_index_reorder_carry(szg_index *ix, const uint64_t *src_rows, uint64_t n_rows,
                            szg_mask *const *masks, int n_masks,
                            szg_column *const *columns, int n_columns);
int szg_index_compact_carry(szg_index *ix, uint64_t *out_new_of_old, uint64_t *out_rows,
                            szg_mask *const *masks, int n_masks,
                            szg_column *const *columns, int n_columns);
typedef struct szg_column_info {
    int32_t kind;            /* SZG_COL_* */
    uint64_t rows;           /* szg_column_rows */
    uint64_t device_bytes;   /* values, present words and heaps as allocated, summed over the parts */
    uint64_t heap_used;      /* text columns: bytes in use, dead ones included, summed over the parts; else 0 */
    uint64_t heap_capacity;  /* text columns: bytes allocated, summed over the parts; else 0 */
} szg_column_info;
int szg_column_get_info(const szg_column *c, szg_column_info *out);   /* works on a stale column */

/* ---- bulk mutations: many rows per call (added under ABI 4, additive) ----
 *
 * szg_index_overwrite, szg_index_overwrite_f64, szg_index_tombstone and szg_column_set for a LIST of rows, with a
 * constant number of device synchronisations per shard and per 64 MiB of the caller's data instead of a round trip
 * per row.  Each call leaves the handle in the state the loop of its single-row form would, with one documented
 * difference: every argument is checked before anything on the card changes, so a bad entry refuses the whole call
 * where the loop would have applied the entries before it.
 * Rows: rows[0 .. n_rows) are numbered as the call's single-row form numbers them (szg_column_set_rows: as
 *   szg_column_set does).  row_bytes, vectors and values are n_rows consecutive entries, entry i for rows[i]:
 *   row_bytes in the reference encoding szg_index_overwrite takes; vectors float64, quantized and packed on the
 *   device exactly as szg_index_overwrite_f64 does; values as szg_column_append's.  present_bits: NULL = every entry
 *   is present; otherwise bit i belongs to rows[i], and the value of an absent entry is ignored -- the row keeps its
 *   stored value and reads as absent, as after szg_column_set(row, NULL).
 * Refusals, nothing changed: a NULL argument (out_dropped and present_bits excepted) is SZG_E_INVALID; a row at or
 *   past the handle's (the column's) rows is SZG_E_RANGE, "row out of range"; a row listed twice is SZG_E_INVALID,
 *   "row listed twice", in the overwrite and the column forms -- szg_index_reorder's rule, which keeps the scatter free
 *   of two writers to one row.  The tombstone forms accept duplicates and rows that are already dead.  n_rows == 0 is
 *   SZG_OK and changes nothing.
 * Overwrites: a tombstoned row may be overwritten and stays dead.  Where the handle keeps row norms or an 8-bit
 *   sketch, the listed rows' norms are refreshed at once -- bit for bit the norms a single-row overwrite leaves -- and
 *   their sketches at the next search; more than 4 096 rows overwritten since the last search rebuild the sketch.
 * Tombstones: *out_dropped (nullable) = the rows that were live before the call and are not afterwards.
 *   szg_index_tombstone_mask drops every live row whose bit is set in `mask`, a current mask of this handle (a stale
 *   or foreign one is SZG_E_INVALID, as in a search); the mask stays valid and unchanged.
 * No call makes a mask or a column stale.
 * Columns: szg_column_set_rows covers SZG_COL_F64 and SZG_COL_U32.  On a text column it is SZG_E_INVALID (the kind
 *   does not match): text values keep szg_column_set_str, row by row -- a bulk form for the text heap is out of scope.
 * Memory: the data travels through the shards' staging blocks, which grow to at most 64 MiB of the caller's data plus
 *   the encoded rows and 12 bytes per row of a chunk.  A failed device allocation is SZG_E_NOMEM with rows, live bits,
 *   norms, sketch bookkeeping, column values and the process's device blocks as they were.
 * A device error (SZG_E_DEVICE) is not covered by "nothing changed": it may leave the update partly applied -- the
 *   shards before the failing one rewritten, the sketch bookkeeping moved -- as a single-row call that fails half-way.
 * These are mutations: callers hold the write lock, as for the single-row forms.
 */
int szg_index_overwrite_rows(szg_index *ix, const uint64_t *rows, const uint8_t *row_bytes, uint64_t n_rows);
int szg_index_overwrite_rows_f64(szg_index *ix, const uint64_t *rows, const double *vectors, uint64_t n_rows);
int szg_index_tombstone_rows(szg_index *ix, const uint64_t *rows, uint64_t n_rows, uint64_t *out_dropped);
int szg_index_tombstone_mask(szg_index *ix, const szg_mask *mask, uint64_t *out_dropped);
int szg_column_set_rows(szg_column *c, const uint64_t *rows, const void *values, const uint64_t *present_bits,
                        uint64_t n_rows);

/* ---- ingest from device memory (added under ABI 4, additive) ----
 *
 * szg_index_append_f64 and szg_index_overwrite_rows_f64 for vectors that already lie in device memory -- the output of
 * an embedding model, a torch tensor -- in float64, float32, float16 or bfloat16.  Every element widens to float64
 * exactly (float32 subnormals included), so the handle ends exactly where the _f64 form would leave it given the same
 * values widened on the host: resident bytes, live bits, row counts, row norms (refreshed at once where the handle keeps
 * them) and sketch bookkeeping.  An append makes masks stale, an overwrite makes nothing stale, a tombstoned row stays
 * dead, columns stay short until szg_column_append.
 * Source: element (r, e) of the source is data[r * row_stride + e], e < the handle's dimension; row_stride counts
 *   elements and is at least the dimension (larger: a column slice of a wider matrix).  data is aligned to its element
 *   size, no more.  src_rows is a HOST array or NULL: NULL = entry i comes from source row i, and n_rows <=
 *   src->n_rows is required; otherwise entry i comes from source row src_rows[i], in any order, duplicates allowed.
 *   The list travels to the card at 8 bytes per row, in chunks of 64 MiB.
 * Refusals, all decided on the host before anything on the card changes (no kernel is launched on a pointer that
 *   failed a check), SZG_E_INVALID unless stated: a NULL argument (src_rows excepted); an unknown dtype; row_stride <
 *   the dimension; data not aligned to its element size; n_rows > src->n_rows without a list; an entry of src_rows at
 *   or past src->n_rows (SZG_E_RANGE); a device ordinal out of range; data that hipPointerGetAttributes does not
 *   report as device memory of `device` ("not device memory": a pointer the runtime does not know counts as host
 *   memory); source rows that do not all lie inside the allocation hipMemGetAddressRange reports -- the last element
 *   addressed is the largest source row used x row_stride + the dimension -- (SZG_E_RANGE); and, for the overwrite
 *   form, szg_index_overwrite_rows's rules: a row at or past the handle's rows is SZG_E_RANGE, a row listed twice
 *   SZG_E_INVALID.  n_rows == 0 checks the descriptor only.
 * Another device: a source on a device other than the target shard's (the append's target, every shard the overwrite's
 *   list reaches) is refused, SZG_E_INVALID, "source on another device" -- no peer copy is made.  Shards that share
 *   the source's device (devices = {0, 0}) are served.
 * Synchronisation: the call synchronises the source's device before it reads (work queued on ANY stream, the
 *   caller's framework's included, has finished) and returns with the rows resident: the caller may free or rewrite
 *   the source as soon as the call has returned.
 * Memory: the encoder reads the caller's memory in place; nothing is copied and the staging block does not grow for
 *   the source.  The overwrite form still stages its linear block of encoded rows (at most 64 MiB) and its lists.
 * There is no _dev form of szg_index_load (an append to an empty handle covers it).  The same descriptor serves the
 *   two reverse directions below: szg_index_fetch_rows_dev WRITES through `data` (the const is the ingest's), and the
 *   _dev searches read their queries through it.
 */
#define SZG_SRC_F64 0
#define SZG_SRC_F32 1
#define SZG_SRC_F16 2
#define SZG_SRC_BF16 3
typedef struct szg_dev_vectors {
    const void *data;      /* device memory, aligned to its element size (szg_index_fetch_rows_dev writes through it) */
    int dtype;             /* SZG_SRC_* */
    int device;            /* HIP ordinal the memory lives on */
    uint64_t n_rows;       /* source rows available (fetch: destination rows available) */
    uint64_t row_stride;   /* elements from one source row to the next, >= dim */
} szg_dev_vectors;
int szg_index_append_dev(szg_index *ix, const szg_dev_vectors *src, const uint64_t *src_rows, uint64_t n_rows);
int szg_index_overwrite_rows_dev(szg_index *ix, const uint64_t *rows, const szg_dev_vectors *src,
                                 const uint64_t *src_rows, uint64_t n_rows);

/* ---- vectors out to device memory, queries from it (added under ABI 4, additive) ----
 *
 * szg_index_fetch_rows_dev: stored vectors decoded into the caller's device memory -- the vector half of GetDocument
 * for whatever follows a search on the card (a re-ranker, diversification, clustering, a hit's vector as the next
 * query) -- without the packed bytes, the host decode and the upload szg_index_read_rows would take.
 * Rows: entry i is stored row rows[i]; `rows` is a HOST list in any order, duplicates allowed (this is a read), numbered
 *   as searches return them (local + row base).  rows == NULL: entry i is row first_row + i (first_row is ignored when a
 *   list is given).  Tombstoned rows are served as stored, as szg_index_read_rows serves them.  The sketch index is
 *   never read.
 * What is written: dst->data[i * row_stride + e], e < the handle's dimension, receives the reference's decodeVector
 *   value of element e of entry i, converted to dst->dtype:
 *     SZG_SRC_F64   that float64, bit for bit (what decoding the bytes of szg_index_read_rows gives);
 *     SZG_SRC_F32   that float64 converted by ONE round-to-nearest-even (a C cast); for a 32-bit handle the stored float;
 *     SZG_SRC_F16 / SZG_SRC_BF16   the float32 value above converted once more, round-to-nearest-even (two roundings,
 *                   what a cast chain double -> float -> half gives);
 *   overflow goes to +-inf and NaN stays NaN, as IEEE 754 says (which NaN is not promised).  Elements e >= dimension of
 *   a destination row (row_stride > dimension: a column slice of a wider matrix) and destination rows >= n_rows are not
 *   touched.
 * Refusals, all decided on the host before any launch (a refused call writes nothing), with the ingest's codes and
 *   words, `dst` checked as a source of n_rows rows: a NULL handle or descriptor; an unknown dtype; row_stride < the
 *   dimension; data not aligned to its element size; n_rows > dst->n_rows; a device ordinal out of range; not device
 *   memory of `device`; destination rows that reach past the allocation (SZG_E_RANGE).  A listed row, or first_row +
 *   n_rows, past the handle's rows is SZG_E_RANGE.  A destination on a device other than that of any shard the rows
 *   reach is SZG_E_INVALID, "destination on another device" -- no peer copy is made; shards that share the
 *   destination's device (devices = {0, 0}) are served.  n_rows == 0 checks the descriptor only.
 * Synchronisation: the call synchronises the destination's device before it writes and returns with the values written
 *   and visible to any stream of that device.
 * Memory: the only upload is the list, 8 bytes per row in chunks of 64 MiB, through a shard's staging block; the kernel
 *   writes the caller's memory in place.
 * Threads: a read, like szg_index_read_rows -- beside searches, not beside mutations.
 *
 * szg_search_topk_dev / szg_search_radius_dev: szg_search_topk_masked / szg_search_radius_masked for queries that lie in
 * device memory.  Query i is source row src_rows[i] (a HOST list or NULL = row i, exactly as in the ingest), every
 * element widened to float64 exactly, and the answer is what the masked call returns for those float64 values -- ids,
 * float64 distances, counts, offsets, order, SZG_E_TRUNCATED -- on every path and under every option, because after
 * the conversion it IS that call: a small kernel on the queries' device writes the dense n_queries x dim float64 batch
 * into a buffer the handle keeps there, one copy brings it into pinned host memory, and the host prepares the queries
 * as ever (under option query_prep the batches of a top-k call through the sketch are prepared on the card, from the
 * float64 batch that goes up for the re-rank; the copy to the host stays: settling and the fall-back read it).  Outputs
 * are host arrays.
 * The queries may lie on ANY device of the process: they are copied, not swept, so nothing is "on another device".
 * Refusals: the descriptor's are the ingest's (n_queries source rows); everything else -- k, radii, masks, stale masks,
 *   capacity, NULL outputs -- is refused by the masked call as today, after the conversion.
 * Synchronisation: the call synchronises the queries' device before it reads; the caller may rewrite the queries once
 *   the call has returned.
 * Threads: as the masked searches, except that the _dev searches of one handle take turns (they share the handle's
 *   conversion buffers for the length of a call).
 */
int szg_index_fetch_rows_dev(szg_index *ix, const uint64_t *rows, uint64_t first_row, uint64_t n_rows,
                             const szg_dev_vectors *dst);
int szg_search_topk_dev(szg_index *ix, const szg_dev_vectors *queries, const uint64_t *src_rows, int n_queries, int k,
                        const szg_mask *const *masks, int n_masks,
                        uint64_t *out_rows, double *out_dist, int32_t *out_count);
int szg_search_radius_dev(szg_index *ix, const szg_dev_vectors *queries, const uint64_t *src_rows, int n_queries,
                          const double *radii, const szg_mask *const *masks, int n_masks,
                          uint64_t *out_rows, double *out_dist, uint64_t capacity, uint64_t *out_offsets);

/*
 * The reference's float64 distance (c.distance, collection.go:596, :812-832) from
 * one query to each listed row, bit-identical to the reference: the gather-by-row
 * primitive for re-ranking candidates of the LSH path (lshtree.go:283-351 calls
 * consider() per candidate id) or any other candidate generator.
 */
int szg_distances(szg_index *ix, const double *query, const uint64_t *rows, uint64_t n_rows,
                  double *out_dist);

/*
 * c.distance(doc_a.Vector, doc_b.Vector) for stored rows: the primitive under
 * computeAverageDistance (collection.go:348-400), which the Go side keeps (it owns the
 * math/rand pair selection and the in-order float64 sum, :372-398).  out_dist[i] is the
 * reference's float64 distance between the decoded rows rows_a[i] and rows_b[i].
 */
int szg_pair_distances(szg_index *ix, const uint64_t *rows_a, const uint64_t *rows_b, uint64_t n_pairs,
                       double *out_dist);

/*
 * Cross-shard result assembly for one-process-per-GPU sharding (host code, no
 * device work).  Every rank answers the batch on its own row range with
 * szg_search_topk asking for list_len = k+1 results (rows made global with
 * szg_index_set_row_base); the per-rank lists are exchanged with one RCCL
 * all-gather and merged here by replaying consider()'s top-k branch
 * (collection.go:606-619) over their union in visit order.
 *   rows/dist  [n_lists][n_queries][list_len], counts [n_lists][n_queries]
 *   out_*      [n_queries][k] (+ out_count[n_queries])
 *   out_history_dependent  nullable, [n_queries]: 1 when two of the best k+1
 *              distances are equal or NaN, i.e. the reference's answer depends
 *              on its whole heap history and a single-handle search over the
 *              unsharded corpus would take the exact-replay path.
 */
int szg_merge_topk(int k, int n_lists, int list_len, int n_queries, const uint64_t *rows,
                   const double *dist, const int32_t *counts, uint64_t *out_rows,
                   double *out_dist, int32_t *out_count, uint8_t *out_history_dependent);
/* The same merge straight from the exchanged buffer, no repacking on the caller's side:
 * records[n_lists][n_queries][2*list_len + 1] int64 = list_len rows | list_len float64 bit
 * patterns | count, i.e. what each rank contributes to the all-gather. */
int szg_merge_topk_records(int k, int n_lists, int list_len, int n_queries, const int64_t *records,
                           uint64_t *out_rows, double *out_dist, int32_t *out_count,
                           uint8_t *out_history_dependent);

/* ---- one process per GPU: the exchange inside the library ----------------- */

/*
 * The loop collection.go:672-684 visits independent records, so the rows shard over the GPUs of a node in
 * contiguous ranges, one process (and one handle) per GPU; szg_index_set_row_base makes the rows a rank returns
 * global.  A sharded search runs the rank's own exact search on its range, exchanges the per-rank results with ONE
 * all-gather per micro-batch -- RCCL (ncclAllGather over xGMI) on the rank's device -- and replays the reference's
 * selection over the union on every rank, so every rank returns the single-collection answer.
 *
 * Set-up: rank 0 calls szg_comm_unique_id and hands the 128 bytes to the other ranks by whatever means the host
 * has (a file, a socket, its own RPC); then EVERY rank calls szg_comm_create (collective: ncclCommInitRank) and
 * attaches the communicator to its handle.  All sharded calls are collective too: every rank makes the same
 * calls, in the same order, with the same queries.  One communicator serves any number of handles of the process.
 */
typedef struct szg_comm szg_comm;
#define SZG_COMM_ID_BYTES 128
int szg_comm_unique_id(uint8_t *id /* [SZG_COMM_ID_BYTES] */);
int szg_comm_create(szg_comm **out, const uint8_t *id, int rank, int world, int device);
/* The same with the host's own transport instead of RCCL: fn all-gathers bytes_per_rank bytes from every rank's
 * `send` into `recv` ([world][bytes_per_rank], rank order) and returns 0.  Host memory only, no device needed
 * (hosts with their own fabric; the tests: gloo on CPU, several ranks on one card). */
typedef int (*szg_allgather_fn)(void *user, const void *send, void *recv, uint64_t bytes_per_rank);
int szg_comm_create_host(szg_comm **out, szg_allgather_fn fn, void *user, int rank, int world);
void szg_comm_destroy(szg_comm *c);
/* Size the exchange staging for micro-batches of up to n_queries queries at this k ahead of time (it grows on
 * demand otherwise -- a hipHostMalloc inside the first call that needs it).  COLLECTIVE like the searches: every
 * rank calls it with the same arguments; the ranks confirm to each other that all of them hold the staging (one
 * status word over the staging that already exists), so a rank that cannot allocate makes EVERY rank return
 * SZG_E_NOMEM here instead of leaving its peers waiting in a later exchange. */
int szg_comm_reserve(szg_comm *c, int n_queries, int k);
/* The handle's sharded searches go through `c` (borrowed: destroy it after the handle, or attach NULL first). */
int szg_index_attach_comm(szg_index *ix, szg_comm *c);

/*
 * szg_search_topk over the sharded collection.  allow_bits covers THIS rank's rows (n_queries x ceil(local rows / 64)
 * words).  More than 128 queries are pipelined in micro-batches of 256: a worker thread sweeps the next one while
 * this thread exchanges and merges.
 * out_history_dependent (nullable, [n_queries]): 1 when two of the best k+1 merged distances are equal or NaN, i.e.
 * the reference's order depends on its whole heap history, which no single rank holds.  With tie_mode 0 (default)
 * such a query is then answered EXACTLY as the unsharded collection would: the heap travels rank 0 -> 1 -> ... in
 * visit order, each rank replaying consider() over its own rows (G more small all-gathers for the flagged queries
 * of the call together), so N > 1 returns what N = 1 returns, order included.
 *
 * Failure semantics of every collective call (this one, szg_search_radius_sharded, szg_comm_merge_*): a rank whose
 * own search or allocation fails still enters every exchange of the call and marks its contribution, so EVERY rank
 * returns an error and none waits for a peer that never comes.  The one case left to the host's own timeout is a
 * transport failure part-way through an exchange (HIP / RCCL error between enqueue and wait on one rank).
 */
int szg_search_topk_sharded(szg_index *ix, const double *queries, int n_queries, int k, const uint64_t *allow_bits,
                            uint64_t *out_rows, double *out_dist, int32_t *out_count, uint8_t *out_history_dependent);
/* szg_search_radius_batch over the sharded collection: an all-gather of the hit counts, one padded all-gather of
 * (row, distance) records, the reference's push-all / pop-all heap over the union in row order.
 * `capacity` may differ between ranks: SZG_E_TRUNCATED (out_offsets complete) is a LOCAL condition -- fetch the
 * answer again with szg_comm_last_radius and a buffer of out_offsets[n_queries] entries; never repeat the
 * collective call on the truncated ranks only. */
int szg_search_radius_sharded(szg_index *ix, const double *queries, int n_queries, const double *radii,
                              const uint64_t *allow_bits, uint64_t *out_rows, double *out_dist, uint64_t capacity,
                              uint64_t *out_offsets);
/*
 * The exchange-and-merge halves on their own (what the two calls above do after the rank's own search): the rank's
 * exact top-(k+1) lists  rows / dist [n_queries][k+1], counts [n_queries]  (rows global)  ->  out_* [n_queries][k];
 * the rank's radius hits in CSR form (offsets [n_queries + 1], rows global, ascending distance per query) -> the
 * merged CSR.  Pure host code plus the transport.
 */
int szg_comm_merge_topk(szg_comm *c, int k, int n_queries, const uint64_t *rows, const double *dist,
                        const int32_t *counts, uint64_t *out_rows, double *out_dist, int32_t *out_count,
                        uint8_t *out_history_dependent);
int szg_comm_merge_radius(szg_comm *c, int n_queries, const uint64_t *offsets, const uint64_t *rows,
                          const double *dist, uint64_t *out_rows, double *out_dist, uint64_t capacity,
                          uint64_t *out_offsets);
/* The merged answer of this communicator's LAST radius call again (not collective): what a rank whose buffer was too
 * small calls after SZG_E_TRUNCATED. */
int szg_comm_last_radius(szg_comm *c, int n_queries, uint64_t *out_rows, double *out_dist, uint64_t capacity,
                         uint64_t *out_offsets);
/*
 * The heap chain on its own (what szg_search_topk_sharded runs for its flagged queries): `replay` continues the
 * reference's heap -- container/heap's array, heap_n entries of (row, distance), element for element -- over THIS
 * rank's rows of flagged query j in visit order (consider()'s top-k branch, collection.go:606-619) and returns 0.
 * Collective: rank g replays in round g.  out_* [n_flagged][k].
 */
typedef int (*szg_replay_fn)(void *user, int j, int k, uint64_t *heap_rows, double *heap_dist, int32_t *heap_n);
int szg_comm_chain_topk(szg_comm *c, int k, int n_flagged, szg_replay_fn replay, void *user, uint64_t *out_rows,
                        double *out_dist, int32_t *out_count);

typedef struct szg_comm_stats {
    uint64_t exchanges;   /* data all-gathers of the searches (ONE per top-k micro-batch, two per radius batch) */
    double exchange_us;   /* wall time inside all all-gathers (copies + collective + wait) */
    double host_us;       /* packing the records and merging the gathered lists */
    int rccl_ranks;       /* ncclCommCount of the communicator (0: host transport) */
    int zero_copy;        /* RCCL: the collective reads / writes the pinned host staging itself (no H2D / D2H copies) */
    uint64_t chained_replays; /* top-k queries whose merged answer held equal distances and was settled by the
                                 rank-to-rank heap chain (the reference's order, collection.go:606-619) */
    uint64_t status_rounds;   /* one-word all-gathers in which the ranks agreed on their staging (only when it grows) */
    uint64_t chain_rounds;    /* all-gathers of the heap chain (world per call that has flagged queries) */
} szg_comm_stats;
int szg_comm_get_stats(szg_comm *c, szg_comm_stats *out);
int szg_comm_reset_stats(szg_comm *c);

/* ---- diagnostics -------------------------------------------------------- */

const char *szg_strerror(int code);
/* Text of the last error raised on the calling thread ("" if none). */
const char *szg_last_error(void);
int szg_abi_version(void);

typedef struct szg_stats {
    uint64_t queries;          /* top-k + radius queries served */
    uint64_t scan_launches;    /* launches of the fused scan kernel */
    uint64_t escalations;      /* top-k queries whose first pass could not be certified */
    uint64_t scan_bytes;       /* bytes swept: rows x row_bytes per pass over the rows -- one pass per query of a
                                  one-sweep launch, or per group of scan_group queries where the launch forms groups;
                                  one per query group of a shared sweep */
    double scan_ms;            /* HIP-event time of the scan kernel launches (timing on) */
    double total_ms;           /* HIP-event time of the whole per-query pipeline (timing on) */
    uint64_t timed_launches;   /* launches included in scan_ms */
    uint64_t full_replays;     /* top-k queries answered by the exact full-history replay
                                  (equal distances or NaN among the best k+1 candidates) */
    uint64_t mq_launches;      /* shared (multi-query) sweeps; each is also one scan launch */
    uint64_t mq_queries;       /* queries answered through shared sweeps */
    uint64_t mq_fallbacks;     /* shared-sweep batches redone through the score matrix (candidate buffer overflow) */
    /* host time of szg_search_topk outside the waits for results (always measured): query
     * preparation (swizzle / digit planes, first-k rows), the HIP calls that enqueue a batch
     * (copies, launches, events: these can block on a full queue), and result assembly
     * (gather, certification, heap replay) */
    double host_prep_us;
    double host_finish_us;
    double host_enqueue_us;
    uint64_t sketch_queries;   /* top-k queries answered through the 8-bit sketch pre-pass ("sketch" option) */
    uint64_t sketch_fallbacks; /* ... that it could not settle and handed to the full-precision path */
    uint64_t mq_bf16_sweeps;   /* shared sweeps that ran on the bfloat16 matrix cores (64- / 32- / 16-bit rows, top-k batches
                                  on 8-bit rows in whole 64-byte steps; their candidates are re-scored in float32 and
                                  re-ranked in float64 like every other path's) */
    uint64_t sketch_radius_queries;   /* radius queries answered through the 8-bit sketch ("sketch_radius" option) */
    uint64_t sketch_radius_fallbacks; /* ... that it handed to the float32 sweep: a zero query under cosine, a non-finite
                                         query or radius, a widened radius that covers everything, more candidates than
                                         the batch's buffers hold */
} szg_stats;

/* HIP-event timing on the library's own streams (off by default): 1 = events around the scan
 * launches (scan_ms / timed_launches), 2 = also around each batch's whole pipeline (total_ms). */
int szg_set_timing(szg_index *ix, int enabled);
int szg_get_stats(szg_index *ix, szg_stats *out);
int szg_reset_stats(szg_index *ix);

/*
 * Top-k searches of large k through the sketch (option sketch_topk_collect): what the path served on the handle since
 * szg_reset_stats, which clears the five counters.  Kept beside szg_stats, whose layout stays as it is (ABI 4, additive):
 * szg_stats.queries and scan_bytes count these searches as they count radius searches through the sketch -- a settled
 * query once, the sample pass as its rows x the sketch's row bytes per launch, the collect sweeps as one pass per launch
 * that shares its row reads and one per query elsewhere.
 */
typedef struct szg_sketch_topk_stats {
    uint64_t queries;      /* top-k queries the path settled */
    uint64_t fallbacks;    /* ... and those it handed to the full-precision path (the option's paragraph lists the reasons) */
    uint64_t sample_rows;  /* rows scored by the sample passes, per launch (not per query) */
    uint64_t candidates;   /* entries the collect sweeps and the staged rows left in the settled queries' buffers */
    uint64_t overflows;    /* of the fallbacks: more candidates than the batch's buffers held */
} szg_sketch_topk_stats;
int szg_index_sketch_topk_stats(szg_index *ix, szg_sketch_topk_stats *out);

/*
 * Option query_prep: which side prepared the queries of the handle's top-k calls through the sketch since szg_reset_stats,
 * which clears the three counters.  A getter of its own beside szg_stats, as szg_index_sketch_topk_stats is.
 */
typedef struct szg_query_prep_stats {
    uint64_t queries_dev;   /* queries of sketch top-k batches that the card prepared */
    uint64_t queries_host;  /* ... and that the host prepared (every one under query_prep = 0) */
    uint64_t launches;      /* launches of the preparing kernel: one per such batch and shard */
} szg_query_prep_stats;
int szg_index_query_prep_stats(szg_index *ix, szg_query_prep_stats *out);

/*
 * Tunables (name, default, meaning): the seventeen a deployment could want.  All are safe to change between calls.
 * (Rounds 1-3 exposed another fifteen -- ring depths, waves per CU, stream placement, sweep kinds per row width --
 * whose values measurement settled; they are compile-time constants now, csrc/scan_internal.h, and A/B runs go
 * through `make variant`.)
 *
 *   answer semantics
 *     tie_mode            0   when two of the best k+1 distances are exactly equal, or one is NaN, the reference's
 *                             output depends on its whole heap history, so the query is re-answered by an exact
 *                             replay over every row; 1 = keep the fast answer (a valid top-k whose order among equal
 *                             distances may differ from the reference's)
 *     slack               16  extra candidates kept beyond k (at least; k/2 when larger)
 *   one sweep per query
 *     queries_per_launch  16  sweeps one scan launch walks back to back (query-major): no launch gap or chip-wide
 *                             tail between the sweeps of a batch
 *     scan_group          0   queries of a launch the one-sweep kernel scores per row read.  8-bit rows (plain 8-bit
 *                             collections and the sketch pre-pass), top-k, no filter and no tombstones, lists in
 *                             registers (kp <= 64): the launch walks its queries in groups of up to this many and reads
 *                             every row once per GROUP.  The 8-bit arithmetic is exact, so keys, lists and answers are
 *                             those of 1, bit for bit.  0 = automatic (4), 1 = one query per row read, 2 / 4 = that
 *                             group size where the launch qualifies; a launch of one query always reads at 1.  Other
 *                             row widths, radius / escalation sweeps, masked launches and longer lists are always 1
 *     scan_group_ring     0   16-byte loads a lane of a grouped launch (scan_group) keeps in flight.  A group of G
 *                             queries spends G times the arithmetic on every piece it loads, so a load has less time
 *                             to return per unit of work than in the kernel without groups; the grouped kernels of
 *                             row shapes with 12 pieces per lane (768 dimensions) therefore exist at two depths, 4
 *                             (the depth of the kernel without groups) and 6.  0 = automatic (6), or one of the two;
 *                             other values are refused.  Launches without groups and the other shapes keep their one
 *                             depth whatever the value.  Keys, lists and answers do not depend on it
 *     scan_norms          0   launches that form groups (scan_group) take every row's norm from a resident array --
 *                             4 bytes per row, brought up to date before the sweep is enqueued when rows were added --
 *                             instead of summing it in the sweep; the value is the same float, so keys do not change.
 *                             0 = automatic, 1 = always sum the norms in the sweep (test and A/B hook; the environment
 *                             variable SZG_NO_ROW_NORMS switches every resident norm off).  Without memory for the
 *                             array the sweep sums the norms; szg_stats.scan_bytes counts row bytes only
 *     sketch_planes       0   int8 digit planes (radix 128) of a query prepared for a sweep of the sketch: 0 = automatic
 *                             (2: |Q| <= 16 000, the quantization step enters the certificate's bound), 3 = |Q| <= 10^6
 *                             as on plain 8-bit handles, which always take 3.  Only queries are prepared differently:
 *                             changing it invalidates nothing resident.  Other values are refused
 *     sketch_matrix       0   the matrix sweep: one-sweep launches over tiled 8-bit rows of whole 64-byte steps whose
 *                             queries carry two digit planes -- the sketch pre-pass -- without filter or tombstones,
 *                             with lists in registers, resident norms and scan_group = 0 score up to 16 queries per
 *                             row read on the matrix cores.  0 = automatic (launches of 3 queries or more; a lone query
 *                             keeps the kernel without groups), 1 = never (the grouped kernels of scan_group), 2 = every
 *                             launch the shape allows, whatever its query count.  Keys stay inside the same error bound
 *                             but are not bit-identical to the grouped kernels'; answers are.  szg_stats.scan_bytes
 *                             counts one pass per 16 queries of such a launch.  Other values are refused
 *     sketch_select       0   how the matrix sweep keeps its 16 lists per wave: 0 = automatic -- lists of up to 16
 *                             entries (sketch_list; 8 by default) live in the 16 lanes of a quarter of the wave, four
 *                             queries to a register pair, and every round inserts one candidate into each of the 16 --,
 *                             1 = one whole-wave list per query and one insert at a time, which longer lists always
 *                             take.  Lists, keys, the drop bound and answers are the same bit for bit; only the
 *                             sweep's time differs.  Other values are refused
 *     sketch_wide         0   the matrix sweep's two-block form: launches of 17 to 32 queries with row lists (sketch_select)
 *                             score 32 queries per row read where both blocks' images and lists fit 64 KiB of LDS (768
 *                             dimensions: lists of up to 15 entries).  0 = automatic: a sketch call of 72 one-sweep queries
 *                             or more under the default query_batch and queries_per_launch takes batches of 32 queries,
 *                             one launch each, between its first and last batch of 4, and settles them on a second host
 *                             thread (finish_thread); 1 = never; 2 = every sketch call of more than 16 queries takes
 *                             batches and launches of up to 32, whatever its length.  Lists, keys, the drop bound and
 *                             answers are the same bit for bit; szg_stats.scan_bytes counts one pass per 32 queries of a
 *                             wide launch.  Other values are refused
 *     sketch_share        0   the matrix sweep's shared form: ONE launch of 33 to 64 queries as two column groups of 32 on
 *                             paired blocks that walk the same rows, so that the second reader of a row finds it on the
 *                             die -- where the two-block form (sketch_wide) serves the shard and it has no dead rows.
 *                             0 = automatic: a sketch call of 136 one-sweep queries or more under the default query_batch
 *                             and queries_per_launch takes batches of 64 queries, one launch each, between its first and
 *                             last batch of 4 (shorter calls keep their plan); 1 = never; 2 = every sketch call of more
 *                             than 32 queries takes batches of up to 64 from its first query on.  Keys and answers are
 *                             the same bit for bit; szg_stats.scan_bytes counts one pass per column group, two for a
 *                             shared launch.  Other values are refused
 *     sketch_bulk         0   crowded tiles of the row lists (sketch_select): a tile of 16 rows whose pre-filter lets
 *                             many (query, row) pairs of a wave through -- a wave's first tiles, while its lists fill --
 *                             merges each list with its 16 candidates whole, by a fixed sorting network, where the
 *                             rounds would insert them one per list and round.  0 = automatic (tiles with 48 passing
 *                             pairs or more), 1 = never (rounds only), n = 2 .. 1024: tiles with n passing pairs or more
 *                             (2: practically every tile that selects; a tile has at most 512 pairs).  Lists, keys,
 *                             the drop bound and answers are the same bit for bit.  Other values are refused
 *     query_batch         16  queries staged, merged, re-ranked and copied back together
 *     mask_dense          1   sweeps whose filter / tombstone masks pass at least half the rows read every row and
 *                             apply the masks at the row finish; selective masks (and 0) compact the row steps that
 *                             hold a passing row first
 *     serialize_scans     1   sweeps of one shard never overlap each other (every sweep has the whole HBM bandwidth)
 *     contexts            4   batches in flight per shard.  A call with one sweep per query uses at most the first
 *                             GPU_MAX_HW_QUEUES - 1 of them (3 at HIP's default of four hardware queues), so that
 *                             the scan stream and every context's stream in use have a hardware queue of their own --
 *                             as far as the runtime hands streams to queues in the order of their creation, which it
 *                             does not promise
 *   sketch pre-pass (float32 rows)
 *     sketch              2   2 = automatic (the default): a handle of float32 rows with >= max(65 536,
 *                             sketch_min_rows) rows keeps an 8-bit sketch of every row (+25 % memory, built on the
 *                             device at the first search after a load, kept up to date across appends / overwrites /
 *                             tombstones) when k + sketch_extra fits the sketch sweep's lists and no test hook is set,
 *                             and answers one-query-per-sweep searches by sweeping the sketch (a quarter of the bytes)
 *                             for candidates, re-ranking those on the float32 rows in float64 and certifying with the
 *                             triangle inequality of the reference's distance; unsettled queries take the full sweep.
 *                             Same answers.  1M x 768 cosine k=10: 2.25 k -> 7.6 k queries/s.  Auto mode steps aside
 *                             -- without an error -- until the next load when the sketch would leave less than an
 *                             eighth of a card's memory (at least 1 GiB) free or an allocation of it fails, and until
 *                             the next mutation or load once 16 of the last 64 queries it took were handed over to the
 *                             full sweep.  1 = always (n >= sketch_min_rows; allocation failures are errors), 0 = never
 *     sketch_extra        30  candidates beyond k; the pre-pass serves k + sketch_extra <= 64
 *     sketch_list         0   entries the sketch sweep keeps per wave and per block (m): 0 = automatic (8 at 512
 *                             blocks, max(8, 2 kp / blocks + 8) in general), >= kp = the full kp-entry lists and the
 *                             two-level merge (the behaviour before short lists).  With m < kp ONE merge launch per
 *                             batch selects the kp best and the drop bound (the smallest m-th entry of a full block
 *                             list), and the certificate takes the lower of it and the kp-th key, so a block holding
 *                             more than m of the best rows sends the query to the full sweep.  Same answers.
 *     sketch_min_rows     4096  collections below this size always take the full sweep
 *     sketch_radius       0   1 = radius queries that would each take a sweep of their own -- a lone szg_search_radius, or
 *                             a batch under radius_mq = 0 -- go through the sketch wherever "sketch" applies to the handle
 *                             (float32 rows, its row-count rule and its steps aside; no rule on k): a collect sweep of the
 *                             sketch at the radius widened by the largest row-to-sketch distance finds every hit by the
 *                             triangle inequality (a quarter of the bytes), the float64 re-rank on the float32 rows and
 *                             `distance <= radius` decide.  Launches of 3 queries or more without filter or tombstones
 *                             share each row read on the matrix cores (16 per read, 32 under the sketch_wide rules;
 *                             szg_stats.scan_bytes counts one pass per 16 / 32 queries of such a launch).  A zero query
 *                             under cosine, a non-finite query or radius, a widened radius of 1 or more under cosine
 *                             and a query with more candidates than the batch's buffers hold take the float32 sweep.
 *                             Same answers.  0 = never (the default): the option is new and off, as the top-k pre-pass
 *                             was -- built as an option, soaked by the fuzzers (scripts/fuzz_gpu.py and
 *                             scripts/fuzz_state.py), made the default by a later change.
 *                             Batches that share a sweep (radius_mq = 1, two queries or more) keep it.  Other values
 *                             are refused
 *     sketch_masked       0   1 = a top-k launch of the sketch pre-pass with tombstones or filter masks (one resident mask
 *                             for every query, per-query resident masks, words from the host) takes the matrix sweep
 *                             wherever the same launch without masks would -- 16 queries per row read, 32 and 64 under the
 *                             sketch_wide and sketch_share rules, the call split as the unmasked call of its size -- with
 *                             a row's eligibility tested where its keys are; a launch whose queries share one mask (or
 *                             have tombstones alone) skips every tile of 16 rows none of which is eligible.  szg_stats.
 *                             scan_bytes counts one pass per group of such a launch.  Same answers.  0 = never (the
 *                             default): masked launches keep the one-query kernel, one pass per query; the option is new
 *                             and off while it soaks, as sketch_radius was.  Radius searches, plain 8-bit handles and
 *                             lists of more than 64 entries stay as they are.  Other values are refused
 *     sketch_f64          0   1 = a handle of 64-bit rows (float64, the reference's default quantization) keeps the 8-bit
 *                             sketch too, under every rule a float32 handle's is under: sketch 0 / 1 / 2, sketch_min_rows,
 *                             the 65 536-row and memory rules of automatic mode, the steps aside, k <= 34; sketch_radius
 *                             and sketch_masked apply to it as they do there.  The sketch is an eighth of the rows'
 *                             bytes (+12.5 % device memory); it is built from the doubles themselves (nothing is
 *                             narrowed to float32: rows of any finite magnitude, subnormal ones included, get their
 *                             nearest bytes), and a query it does not settle takes the handle's own 64-bit sweep.  Same
 *                             answers, the reference's float64 distances bit for bit.  szg_stats.sketch_queries /
 *                             sketch_fallbacks (and the sketch_radius_ pair) count on the handle as on a float32 one.
 *                             0 = never (the default while the option soaks): a 64-bit handle keeps no sketch, allocates
 *                             nothing more and takes the paths it took before the option existed; set back to 0, the
 *                             handle behaves as a float32 handle does under sketch = 0 (an existing sketch index stays
 *                             until the handle is closed or reloaded).  Handles of other widths ignore it.  Other values
 *                             are refused
 *     sketch_topk_collect 0   1 = a top-k call that takes one sweep per query (a lone szg_search_topk, any call under
 *                             multi_query = 0) with a k the pre-pass does not serve (k + sketch_extra beyond its lists: k >= 35
 *                             by default) goes through the sketch all the same, wherever "sketch" applies to the handle's
 *                             rows (float32, or float64 under sketch_f64 = 1; the row-count rule, the steps aside) and the
 *                             sample plan serves every shard (szg_debug_sample_plan: k <= 2048 and at least 4 k rows in
 *                             every second tile of 16): a SAMPLE pass scores every stride-th tile (stride 16, 8, 4 or 2)
 *                             of the sketch on the matrix cores, 16 or 32 queries per row read; the (k + e)-th smallest
 *                             sample key of a shard (e = its eligible sampled rows without a usable sketch) bounds the
 *                             query's k-th distance from above by tau; a radius search at tau through the sketch -- the
 *                             collect sweep, float64 re-rank and gather of sketch_radius, whatever that option says --
 *                             contains the whole answer, ties included, and the reference's heap is replayed over it.
 *                             A NaN among the first k rows or distances that tie among the best k + 1 (tie_mode = 0), a
 *                             zero query under cosine, a non-finite query, tau widened to 1 or more under cosine, no shard
 *                             with k + e eligible sample rows and more candidates than the batch's buffers hold take the
 *                             full-precision path, all of a call as ONE call (szg_index_sketch_topk_stats counts them;
 *                             they do not enter automatic mode's window).  Same answers.  0 = never (the default while
 *                             the option soaks): no allocation, no launch, one test of the option.  Calls that share a
 *                             sweep (multi_query = 1, mq_min queries or more) keep it.  Other values are refused
 *     query_prep          0   the queries of a top-k call through the sketch (szg_search_topk and its _masked and _dev forms,
 *                             coalesced lone callers) are prepared ON THE CARD: a small kernel per batch and shard turns the
 *                             float64 batch that is uploaded for the re-rank anyway into the sweep's 8-bit image and the
 *                             five constants of each query, by the rule the host follows (csrc/query_prep.h: the same
 *                             bytes and the same bit patterns, the two order-sensitive sums added in element order), the
 *                             sweeps read the constants where the kernel wrote them, and the host receives them, for the
 *                             certificates, by the time it settles the batch.  Keys, lists, certificates and answers are
 *                             the same bit for bit.  0 = never (the default while the option soaks): the host prepares
 *                             every query, no allocation, no launch; 1 = batches of 8 queries or more (a lone search and
 *                             the 4-query edges of a long call stay on the host: a launch would sit in front of their few
 *                             sweeps); 2 = every batch, from one query on (the tests' setting).  Not covered, prepared on
 *                             the host whatever the value: radius searches and sketch_topk_collect calls (they need the
 *                             constants before their sweeps), the full-precision fall-back, shared sweeps (multi_query),
 *                             plain 8-bit and 4-bit handles.  szg_index_query_prep_stats counts both sides.  Other values
 *                             are refused
 *   shared sweeps
 *     multi_query         1   batches of >= mq_min queries share ONE sweep of the corpus, the dot products on the
 *                             matrix cores: 64- / 32- / 16-bit rows on bfloat16 roundings (v_mfma_f32_16x16x32_bf16,
 *                             up to 96 queries per pass; candidates scored again in float32, certified against the
 *                             bfloat16 bound) -- and top-k batches of more than 48 queries on 8-bit rows in whole 64-byte steps, whose codes
 *                             are exact in bfloat16 (only the query is rounded) --, 4-bit rows, the other 8-bit
 *                             shapes and every radius batch on 8-bit rows in exact integer arithmetic
 *                             (v_mfma_i32_16x16x64_i8, 48 per pass, two passes per launch); 0 = no shared sweep on
 *                             the matrix cores: the one-sweep kernel, which on 8-bit rows scores up to scan_group
 *                             queries of a launch per row read
 *     mq_min              2   smallest batch worth a shared sweep
 *     mq_hits             1024 candidates per query the threshold from the prefix pass aims at
 *     coalesce            1   concurrent szg_search_topk calls with ONE query each -- the reference's Searches under
 *                             RLock -- are answered together, up to 96 per shared sweep, by whichever caller finds no
 *                             batch in flight; concurrent szg_search_radius callers likewise
 *     radius_mq           1   radius batches of two or more queries share ONE sweep of the corpus per up to 96
 *                             queries (the radius is the collect threshold); 0 = one collect sweep per query
 *     finish_thread       1   a call of three or more shared-sweep batches assembles its finished batches on a
 *                             second host thread while the caller's prepares and enqueues the next ones
 *   test hooks (paths that data takes by itself only rarely): force_escalate, force_matrix (the score-matrix form of
 *   the shared sweeps: small shards, candidate-buffer overflow), force_no_refine (their tail as separate launches: kp > 256),
 *   force_sketch_nomem (the sketch's device allocation is refused: auto mode steps aside, sketch = 1 reports it),
 *   carry_stage_bytes (the staging window of carried columns on a handle of several shards: 0 = 64 MiB, else a multiple
 *   of 16 up to that, so that a small column travels in several windows)
 */
int szg_set_option(szg_index *ix, const char *name, int64_t value);

/* ---- bench / test utilities (not part of the drop-in surface) ----------- */

/*
 * Fill the mirror with n_rows synthetic vectors generated on the device:
 * element e of row r = U[-1,1) from splitmix64(seed + (first_row + r)*dim + e),
 * quantized and packed exactly as encodeDocument would (collection.go:713-743,
 * quantization.go:5-23).  Byte-identical to oracle/orc_synth_rows.
 */
int szg_index_synth(szg_index *ix, uint64_t n_rows, uint64_t seed, uint64_t first_row);

/* Global row index of this handle's row 0 (multi-process sharding); rows
 * returned by szg_search_* are local + base. */
int szg_index_set_row_base(szg_index *ix, uint64_t base);

/* Test hook: what = 1: the next `value` growths of this rank's exchange staging fail (SZG_E_NOMEM), as an allocation
 * failure on ONE rank of a job would. */
int szg_comm_debug_inject(szg_comm *c, int what, int value);

/*
 * Test hook, host only (no device is touched): how the one-sweep scan would walk n_rows rows of (dim, quant_bits) --
 * computed by the functions the launch path itself calls.  kp: candidates kept per list (k + slack; ignored for a
 * collect sweep), collect: a radius / escalation sweep, masked: a filter mask or tombstones are present, cu_count:
 * compute units of the card (0 = 256).  SZG_E_INVALID / SZG_E_UNSUPPORTED as szg_index_create.
 */
typedef struct szg_scan_plan {
    int32_t r16;            /* 16-byte pieces per row */
    int32_t L, P, gpw;      /* lanes per row, pieces per lane, rows per wave step */
    int32_t pow2;           /* L is a power of two */
    int32_t dense;          /* L*P == r16 and gpw*L == 64 */
    int32_t tiled;          /* rows live in 16-row tiles */
    int32_t grid, block;    /* launch geometry */
    int32_t ring_depth;     /* 16-byte loads each lane keeps in flight */
    int32_t shaped;         /* 0, or L*100 + P of the row-shape-specialised kernel */
    int32_t nontemporal;    /* rows are loaded past the caches */
    int32_t rows_per_block; /* rows one block covers per wave step */
} szg_scan_plan;
int szg_debug_scan_plan(int dim, int quant_bits, uint64_t n_rows, int kp, int collect, int masked, int cu_count,
                        szg_scan_plan *out);

/*
 * Test hook, host only: how a one-sweep call of n_queries queries forms groups (option scan_group) -- by the functions
 * the launch path calls.  The call is split into launches of queries_per_launch queries; *group = the group size of the
 * first launch, *lds_bytes = the LDS that launch asks for, *passes = passes over the rows of the whole call.
 */
int szg_debug_scan_group(int dim, int quant_bits, int kp, int collect, int masked, int scan_group, int n_queries,
                         int queries_per_launch, int32_t *group, uint64_t *lds_bytes, int32_t *passes);

/*
 * Test hook, host only: does the matrix sweep (option sketch_matrix) serve a one-sweep top-k call of n_queries queries,
 * split into launches of 16?  planes = digit planes of the queries (2 or 3), norms = the rows' norms are resident,
 * tiled = 0 takes the tiled layout away, masked = a filter or tombstones.  *serves / *steps_form / *lds_bytes describe
 * the first launch (steps_form: 12 or 6 = the kernel of that many 64-byte steps per row, 0 = the any-steps kernel),
 * *passes = passes over the rows of the whole call.
 */
int szg_debug_scan_matrix(int dim, int quant_bits, int n_queries, int kp, int planes, int norms, int tiled, int masked,
                          int scan_group, int sketch_matrix, int32_t *serves, int32_t *passes, uint64_t *lds_bytes,
                          int32_t *steps_form);

/*
 * Test hook, host only: which selection (option sketch_select) the first launch of a one-sweep top-k call of n_queries
 * queries takes, under the conditions of szg_debug_scan_matrix.  *serves = the matrix sweep serves the launch;
 * *row_lists = 1: it keeps row lists (kp <= 16 under sketch_select = 0), 0: the serial inserts -- or it does not serve.
 */
int szg_debug_scan_select(int dim, int quant_bits, int n_queries, int kp, int planes, int norms, int tiled, int masked,
                          int scan_group, int sketch_matrix, int sketch_select, int32_t *serves, int32_t *row_lists);

/*
 * Test hook, host only: the matrix sweep's two-block form (option sketch_wide) for a one-sweep top-k call of n_queries
 * queries, under the conditions of szg_debug_scan_select, split as a call with wide batches splits it: launches of up to
 * 32 queries where a launch of 32 qualifies for the form, of up to 16 where it does not.  *serves = 1: the first launch
 * scores 32 queries per row read; *lds_bytes = the LDS it asks for -- with b column blocks, 16 b (2 dim64 + 12 +
 * 8 waves kp), dim64 the row bytes in whole 64-byte steps; *passes = passes over the rows of the whole call.
 */
int szg_debug_scan_wide(int dim, int quant_bits, int n_queries, int kp, int planes, int norms, int tiled, int masked,
                        int scan_group, int sketch_matrix, int sketch_select, int sketch_wide, int32_t *serves,
                        int32_t *passes, uint64_t *lds_bytes);

/*
 * Test hook, host only: the matrix sweep's shared form (option sketch_share) for a one-sweep top-k call of n_queries
 * queries through the sketch, under the conditions of szg_debug_scan_wide and the default query_batch and
 * queries_per_launch.  *serves = 1: a launch of min(n_queries, 64) queries takes the shared form (33 queries or more);
 * *slices = the row slices S of such a launch (its grid is 2 S, each query gets S block lists), 0 where it does not
 * serve; *lds_bytes = that launch's LDS.  The call as it is split: batches[0 .. min(*n_batches, batch_capacity)) = the
 * queries of its batches, *launches = its scan launches, *passes = its passes over the rows (two per shared launch).
 */
int szg_debug_scan_share(int dim, int quant_bits, int n_queries, int kp, int planes, int norms, int tiled, int masked,
                         int scan_group, int sketch_matrix, int sketch_select, int sketch_wide, int sketch_share,
                         int32_t *serves, int32_t *launches, int32_t *passes, int32_t *slices, uint64_t *lds_bytes,
                         int32_t *batches, int32_t batch_capacity, int32_t *n_batches);

/*
 * Test hook, host only: the matrix sweep's masked forms (option sketch_masked) for a one-sweep top-k call of n_queries
 * queries through the sketch whose launches carry masks, with the arguments of szg_debug_scan_share plus the option and
 * shared_mask (1: the launch's queries share one mask or have tombstones alone -- its eligibility is wave-uniform; 0:
 * per-query masks).  *serves = 1: a launch of min(n_queries, 64) queries takes a masked form; *wide / *share: that launch
 * takes the two-block / the shared form; *tile_skip: it skips tiles without an eligible row (serves and shared_mask);
 * *steps_form: its kernel's 64-byte steps per row (12, 6, 0 = the any-steps kernel);
 * *launches / *passes: the call's scan launches and passes over the rows as it is split -- with the option off, or where
 * the form does not serve, launches of up to 16 and one pass per query.  masked = 0 describes the call without masks:
 * no masked form (*serves = 0), the launches and passes of szg_debug_scan_share.
 */
typedef struct szg_scan_masked_plan {
    int32_t serves, wide, share, tile_skip, steps_form, launches, passes;
} szg_scan_masked_plan;
int szg_debug_scan_masked(int dim, int quant_bits, int n_queries, int kp, int planes, int norms, int tiled, int masked,
                          int scan_group, int sketch_matrix, int sketch_select, int sketch_wide, int sketch_share,
                          int sketch_masked, int shared_mask, szg_scan_masked_plan *out);

/*
 * Test hook: what the masked forms of the matrix sweep (option sketch_masked) served on the handle's sketch index since
 * szg_reset_stats: launches that took one, those of them with the tile skip, and the queries of all of them.  Zeros for
 * a handle without a sketch.
 */
typedef struct szg_sketch_masked_info {
    uint64_t launches, skip_launches, queries;
} szg_sketch_masked_info;
int szg_debug_sketch_masked(szg_index *ix, szg_sketch_masked_info *out);

/*
 * Test hook, host only: does the matrix sweep's collect form (radius searches through the sketch, option sketch_radius)
 * serve a collect call of n_queries queries with one sweep each, under the conditions of szg_debug_scan_matrix?  The
 * call is split into launches of up to 32 queries where sketch_wide = 2 and a launch of 32 qualifies for the two-block
 * form, of up to 16 otherwise.  *serves / *wide / *steps_form / *lds_bytes describe the first launch (wide: it scores 32
 * queries per row read; lds_bytes: 16 b (2 dim64 + 16) with b column blocks), *passes = passes over the rows of the
 * whole call: one per launch the form serves, one per query elsewhere.
 */
int szg_debug_scan_collect(int dim, int quant_bits, int n_queries, int planes, int norms, int tiled, int masked,
                           int scan_group, int sketch_matrix, int sketch_wide, int32_t *serves, int32_t *wide,
                           int32_t *passes, uint64_t *lds_bytes, int32_t *steps_form);

/*
 * Test hook, host only: the sample plan of a top-k search through the sketch (option sketch_topk_collect; csrc/sample_plan.h)
 * for a shard of shard_rows rows of dim elements at quant_bits (the sketch index is 8; any other width is not served),
 * queries of `planes` digit planes (the sketch's are 2) and a launch of n_queries (1 .. 32).  serves = 0: the shard is
 * not served (untiled rows -- dim no multiple of 64 --, an image beyond 64 KiB of LDS, k beyond 2048, fewer than 4 k rows
 * in every second tile) and the other fields are 0.  stride: in tiles of 16 rows, the largest of 16, 8, 4, 2 that leaves
 * sample_rows >= 4 k; tiles: the sample's; slots = 16 tiles: key slots per query (a partial last tile in the sample
 * keeps all 16); key_bytes = 4 n_queries slots; cap: entries per query the collect buffers start with, 8 k stride rounded
 * up to a power of two; blocks: column blocks of 16 queries the launch scores per row read (1 or 2); lds_bytes: its LDS.
 */
typedef struct szg_sample_plan {
    int32_t serves, stride, blocks, reserved;
    uint64_t tiles, sample_rows, slots, key_bytes, cap, lds_bytes;
} szg_sample_plan;
int szg_debug_sample_plan(uint64_t shard_rows, int k, int n_queries, int dim, int quant_bits, int planes, szg_sample_plan *out);

/*
 * Test hook, host only: *fits = the sketch sweep's one-launch short-list merge serves n_lists block lists of m entries
 * at kp candidates; *sorts = the most entries under its threshold (the kp-th smallest first entry) that its selection
 * sorts in one network -- with more, and always when *sorts < kp, the launch runs the tournament.
 */
int szg_debug_merge_short_plan(int n_lists, int m, int kp, int32_t *fits, int32_t *sorts);

/*
 * Test hook, host only: *ring_depth = the ring depth the launch of a one-sweep call of n_queries (<= 16) queries takes
 * under options scan_group and scan_group_ring; depths[0 .. *n_depths) (room for 2) = the values of scan_group_ring the
 * library accepts beside 0.
 */
int szg_debug_scan_group_ring(int dim, int quant_bits, int kp, int scan_group, int n_queries, int scan_group_ring,
                              int32_t *ring_depth, int32_t *depths, int32_t *n_depths);

/*
 * Test hook, host only: would szg_set_option accept `value` for the one-sweep kernel's option `name` (scan_group,
 * scan_group_ring, scan_norms, sketch_planes, sketch_matrix, sketch_select, sketch_wide, sketch_share, sketch_bulk, sketch_radius,
 * sketch_masked, sketch_f64, sketch_topk_collect, query_prep)?  SZG_OK, or SZG_E_INVALID with szg_set_option's text; any other name is refused.
 */
int szg_debug_option_check(const char *name, int64_t value);

/*
 * Test hook: *out = what option `name` of szg_set_option holds -- on the handle (on_sketch = 0) or on its internal sketch
 * index (on_sketch = 1: SZG_E_UNSUPPORTED while there is none; never a sync).  "contexts" reads as the contexts in rotation
 * on the first shard that has any, that is the free ones: call while no search is in flight.  An unknown name is refused
 * with szg_set_option's text.
 */
int szg_debug_option_get(szg_index *ix, const char *name, int on_sketch, int64_t *out);

/*
 * Test hooks of option query_prep.
 *   szg_debug_query_prep         the images (n_queries x 48 * ceil(dim / 16) bytes: three planes of 16 bytes per 16-byte
 *                                piece of a sketch row, whatever sketch_planes says) and constants (out_meta:
 *                                n_queries x 5 doubles: qnorm, m1, qscale, qconst, qnorm2) that a sweep of the handle's
 *                                sketch would be given for these queries, prepared by the host (on_card = 0) or by the
 *                                kernel (1) -- through the search path's own scaling and launch wrapper.  Brings the sketch
 *                                up to date first, as a search does; SZG_E_UNSUPPORTED on a handle without a sketch.
 *   szg_debug_query_prep_serves  host only: does the card prepare a batch of batch_queries queries under the option's value
 *                                (1 / 0)?  *out_min, if not NULL, receives the smallest batch that value 1 serves.
 */
int szg_debug_query_prep(szg_index *ix, const double *queries, int n_queries, int on_card, uint8_t *out_image,
                         double *out_meta);
int szg_debug_query_prep_serves(int option, int batch_queries, int *out_min);

/*
 * Test hook, host only: *eps = the bound on |scan key - real-number key| that certification uses for a key `key` (in
 * the key's units: -cos, or squared distance times maxInt^2 for rows of 16 bits or fewer) of a collection of dim
 * elements, quant_bits and metric, for the arithmetic `family` -- 0 the one-sweep kernel, 1 the int8 shared sweep, 2 the
 * bfloat16 shared sweep, 3 the float32 shared sweep.  planes: the digit planes of the one-sweep 8-bit query (2 on a
 * sketch index, else 3); mq_planes: those of the int8 shared sweep's query (0: this build's); qnorm, qnorm2: |g| and |g|^2 of the prepared query g (q / |q|, maxInt q, or q); qscale,
 * mq_qscale: the quantization step of the one-sweep integer query and of the int8 shared sweep's.  The arithmetic is
 * csrc/key_bound.h's, the one every search uses.
 */
int szg_debug_key_eps(int dim, int quant_bits, int metric, int planes, int mq_planes, int family, double key, double qnorm,
                      double qnorm2, double qscale, double mq_qscale, double *eps);

/*
 * Test hook, host only: the checks szg_index_reorder makes on its list before anything moves, and the split of the
 * new rows over n_shards shards -- the same code, the same return codes and error text.  live_words: ceil(n_rows / 64)
 * words, bit r == 0 -> row r is tombstoned (NULL: every row is live); src_rows[0 .. n): the list (no row base);
 * out_counts: nullable, n_shards entries.
 */
int szg_debug_reorder_plan(uint64_t n_rows, const uint64_t *live_words, const uint64_t *src_rows, uint64_t n,
                           int n_shards, uint64_t *out_counts);

/*
 * Test hook, host only: the checks the bulk mutations make on their list before anything changes, and its split over
 * the shards of a handle of n_rows rows freshly loaded on n_shards shards -- the same code, the same return codes and
 * error text.  rows[0 .. n): the list, rows[i] - row_base the row; allow_duplicates: 0 = the overwrite and column forms
 * ("row listed twice"), 1 = the tombstone form.  Every out_ pointer is nullable.  out_counts[n_shards]: the entries
 * that fall into each shard; out_local[n] / out_source[n]: the shards' lists back to back, shard 0's first, each in
 * the caller's order -- the shard-local row, and the position i it had in rows[]; out_word_lo / out_word_hi[n_shards]:
 * the first and last 64-row word of the shard that holds a listed row (lo > hi: none).
 */
int szg_debug_bulk_plan(uint64_t n_rows, uint64_t row_base, const uint64_t *rows, uint64_t n, int n_shards,
                        int allow_duplicates, uint64_t *out_counts, uint64_t *out_local, uint64_t *out_source,
                        uint64_t *out_word_lo, uint64_t *out_word_hi);

/*
 * Test hooks, host only: the device memory this process's handles, columns and masks own.  Every device block of theirs
 * -- rows, live bits, norms, staging, column parts, mask words, per-batch scratch -- comes from one function, which
 * counts them (pinned host memory and the one-process-per-GPU exchange's staging are not counted):
 *   szg_debug_device_memory       the blocks alive now and their bytes (either pointer may be NULL);
 *   szg_debug_refuse_device_alloc the nth device allocation from now on (nth >= 1) is refused before the device is
 *                                 asked: its call returns SZG_E_NOMEM with "(refused: test hook)" in the error text, and
 *                                 the countdown disarms itself.  0 disarms.  Process-wide: not for concurrent callers.
 */
int szg_debug_device_memory(uint64_t *out_blocks, uint64_t *out_bytes);
int szg_debug_refuse_device_alloc(int64_t nth);

/*
 * Test hook: the certificate trace.  Every answer is exact because of a chain of bounds (a sweep's float32 key is
 * within key_eps of the real-number key; every row a pass left out has a real-number key at or above the bound the
 * host derives; a collect sweep returns every row under its threshold; the sketch pre-pass's triangle inequality).
 * With the trace on, a handle keeps what each pass handed to certification -- the values the code used -- so that a
 * test can check each bound against float64, row by row.
 *
 *   szg_debug_trace_certificates(ix, on)   per handle, off by default; switching it on (or off) clears what was kept.
 *                                          Off, a settled query pays one branch and nothing is allocated.
 *   szg_debug_certificates(...)            the records of the calls made since, in the two-call style: with records ==
 *                                          NULL or entries == NULL only the three counts are written; with buffers at
 *                                          least as large as the counts the records are copied out and the trace is
 *                                          emptied (SZG_E_TRUNCATED, nothing copied or cleared, when either is smaller).
 *                                          *out_dropped: records that did not fit the handle's caps (2^18 records,
 *                                          2^23 entries) since the trace was switched on; such a record is dropped whole, before its
 *                                          entries are gathered (the bound covers the temporary copies too).
 *
 * One record per settled query per pass; its entries are entries[first_entry .. first_entry + n_entries).  A collect
 * pass run for one query on its own (escalation, a radius query swept again) writes one record per shard; rows
 * [row_lo, row_hi) are the rows the record speaks for.  Safe beside finish_thread and coalesce (the trace has its own lock).
 */
#define SZG_CERT_TOPK 0          /* first top-k pass: keys = ListKeys of the pass */
#define SZG_CERT_SKETCH 1        /* sketch pre-pass (recorded on the float32 -- sketch_f64: float64 -- handle) */
#define SZG_CERT_ESCALATION 2    /* the collect sweep of a query whose first pass was not certified */
#define SZG_CERT_RADIUS_SINGLE 3 /* radius collect, one sweep per query */
#define SZG_CERT_RADIUS_SHARED 4 /* radius collect, one shared sweep per batch */
#define SZG_CERT_SKETCH_RADIUS 5 /* radius collect on the sketch (recorded on the float32 / float64 handle, one record per query):
                                    thr / eps of the sketch sweep, D = the sketch-distance radius R (1 + 1e-9) + slack,
                                    keyed entries = the collected sketch rows with their sketch keys, NO_KEY entries =
                                    the rows without a usable sketch re-ranked beside them */
#define SZG_CERT_SKETCH_TOPK_COLLECT 6 /* top-k of large k through the sketch (option sketch_topk_collect; recorded on the float32 /
                                    float64 handle, one record per settled or handed-over query): thr / eps / D / slack as
                                    for SZG_CERT_SKETCH_RADIUS, of the collect sweep at radius tau; kmax = U, the bound on the
                                    real-number sketch key of k eligible sampled rows; thr_min = tau, the radius U implies
                                    (+ slack); k; certified 1 = settled, 0 = handed over (before the sweep, or with more
                                    candidates than the buffers held: thr, eps, D NaN and no entries).  Keyed entries = the collected sketch rows, NO_KEY entries = the rows
                                    without a usable sketch and the query's first k eligible rows */
#define SZG_CERT_KEYS_SINGLE 0
#define SZG_CERT_KEYS_SHARED_INT8 1
#define SZG_CERT_KEYS_SHARED_BF16 2
#define SZG_CERT_KEYS_BF16_BAND 3
#define SZG_CERT_KEYS_BF16_RESCORED 4
#define SZG_CERT_ENTRY_NO_KEY 1u /* entry flag: a row re-ranked beside the lists (sketch: first-k / unsketched rows) */
typedef struct szg_cert_record {
    int32_t query;       /* index of the query in its call */
    int32_t pass;        /* SZG_CERT_* */
    int32_t keys;        /* top-k and sketch passes: SZG_CERT_KEYS_* (which arithmetic made the list keys); else -1 */
    int32_t sweep;       /* the sweep that ran: 0 one per query, 1 shared on the int8 cores, 2 shared on the bfloat16 cores */
    int32_t certified;   /* top-k: the first pass was certified; sketch: it settled the query (0: handed over); else -1 */
    int32_t k;           /* top-k and sketch passes; else -1 */
    uint64_t row_lo, row_hi;  /* rows of the handle the record speaks for (no row base) */
    double thr_min;      /* top-k: the bound on the real-number key of every eligible row outside the candidates
                            (+inf: every eligible row is among them); sketch: lb, that bound on the sketch keys; else NaN */
    double kmax;         /* top-k: upper bound of the real-number key of the worst result (-inf: not computed); else NaN */
    double thr;          /* collect passes: the key threshold of the sweep; else NaN */
    double eps;          /* collect passes: the sweep's key bound at the threshold -- a row with a real-number key at or
                            below thr - eps is surely collected (computed for the trace, as ub below); else NaN */
    double D, slack;     /* sketch: the distance lb implies and the largest row-to-sketch distance (D NaN: lb infinite) */
    uint64_t first_entry, n_entries;
} szg_cert_record;
typedef struct szg_cert_entry {
    uint64_t row;        /* row of the handle (no row base) */
    double dist;         /* the reference's float64 distance */
    double ub;           /* key + the bound of the arithmetic that made it: what the host takes the real-number key to
                            be at most (collect passes: computed for the trace, by the function certification uses) */
    float key;           /* the sweep's float32 key */
    uint32_t flags;      /* SZG_CERT_ENTRY_* */
} szg_cert_entry;
int szg_debug_trace_certificates(szg_index *ix, int on);
int szg_debug_certificates(szg_index *ix, szg_cert_record *records, uint64_t record_capacity, szg_cert_entry *entries,
                           uint64_t entry_capacity, uint64_t *out_records, uint64_t *out_entries, uint64_t *out_dropped);

/*
 * Test hook: the state of the 8-bit sketch index of a float32 handle -- or of a float64 one, which keeps a sketch under
 * sketch_f64 = 1 -- (option "sketch"), read only.  A
 * settled answer rests on the sketch bytes, on max_ang >= d(row, its sketch) and on the exception list; with these two
 * calls a test checks each against float64.  Neither call brings the sketch up to date or builds one: a test searches
 * first and looks at in_sync.  Both take the lock of the sync, allocate nothing on the device beyond what
 * szg_index_read_rows does, and return SZG_E_INVALID on a NULL argument or a handle whose rows are neither float32 nor
 * float64.
 *
 *   szg_debug_sketch_info(ix, out, exc_rows, exc_capacity)   *out is always written.  In the two-call style: with
 *                                          exc_rows == NULL only *out is written; with exc_capacity >= out->n_exc the
 *                                          rows without a usable sketch are copied out, ascending (SZG_E_TRUNCATED
 *                                          when it is smaller).
 *   szg_debug_sketch_rows(ix, first_row, n_rows, out, live_words, live_capacity)
 *                                          the sketch rows [first_row, first_row + n_rows) in the reference's packed
 *                                          8-bit form, dim bytes each: szg_index_read_rows on the sketch index
 *                                          (SZG_E_RANGE beyond the sketch's rows or without a sketch).  live_words, where
 *                                          not NULL, receives the live words of the sketch shards, index-level,
 *                                          ceil(rows / 64) of them (SZG_E_TRUNCATED when live_capacity is smaller).
 */
typedef struct szg_sketch_info {
    int32_t exists;      /* the handle holds a sketch index */
    int32_t in_sync;     /* ... and it was synced at the handle's current state (no mutation since) */
    int32_t disabled;    /* too many rows without a usable sketch: the sketch index was given back */
    int32_t n_shards;    /* shards of the sketch index (0 without one) */
    uint64_t rows;       /* rows of the sketch index (0 without one) */
    double max_ang;      /* the largest d(row, its sketch) the builds reported */
    double gscale;       /* Euclidean collections: the one scale of every sketch row (0: cosine) */
    uint64_t n_exc;      /* rows without a usable sketch */
} szg_sketch_info;
int szg_debug_sketch_info(szg_index *ix, szg_sketch_info *out, uint64_t *out_exc_rows, uint64_t exc_capacity);
int szg_debug_sketch_rows(szg_index *ix, uint64_t first_row, uint64_t n_rows, uint8_t *out, uint64_t *out_live_words,
                          uint64_t live_capacity);

#ifdef __cplusplus
}
#endif
#endif /* SYZGY_SCAN_H */
