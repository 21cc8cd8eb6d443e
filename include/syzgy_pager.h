/*
 * syzgy_pager.h -- C ABI of the spanfile pager: reads a SyzgyDB collection file
 * (.dat) into the dense rows x row_bytes matrix + row -> document-id table the
 * scan (syzgy_scan.h) works on, without the Go runtime.
 *
 * It restates the READ side of the reference's storage layer, nothing else:
 *   spanfile.go:1-22     span grammar (magic, u32 length, 7-code sequence number,
 *                        record id, streams, padding, CRC32-IEEE trailer)
 *   spanfile.go:282-357  scanFile: walk spans from offset 0; magic 0 = rest is
 *                        free; a span with a bad checksum or parse error is
 *                        skipped by its length; FREE spans are skipped; for a
 *                        record id seen twice the HIGHEST sequence number wins
 *   spanfile.go:568-661  7-code varints (MSB-first base-128)
 *   spanfile.go:730-849  parseSpan / verifyChecksum
 *   collection.go:241-272 the header record "" holds the CollectionOptions JSON,
 *                        :446-450 stream 0 = metadata, stream 1 = packed vector
 *   spanfile.go:540-560  rows come out in IterateSortedRecords order
 *                        (sort.Strings over the decimal record ids)
 *
 * The read rules, as tests/spanfile_model.py restates them and tests/test_pager_malformed_cpu.py holds this to:
 *   walk      stops when fewer than 15 bytes remain, at magic 0, at a length that runs past the end of the file and
 *             at length 0; any other span advances the walk by its length, whatever its magic.
 *             DEVIATION: at length 0 the reference refuses the file ("length is 0; can't continue"); the pager keeps
 *             what it has read up to there.
 *   skipped   counts every ACTIVE span that contributes nothing: shorter than 15 bytes, CRC32-IEEE over length - 4
 *             bytes different from the trailer, or a structure that does not fit the span -- a 7-code that runs to
 *             the span end, an id or stream that ends past it (compared in true arithmetic: a length near 2^64 does
 *             not wrap into range), a missing stream-count or stream-id byte, fewer than 4 bytes left for the trailer.
 *             A 7-code's value is the reference's uint64 arithmetic (modulo 2^64), the sequence number that modulo 2^32.
 *             A record that parses and is not served (below) is NOT counted.
 *   winner    per record id (as bytes) the strictly highest sequence number; on equal numbers the earlier span stays.
 *   header    fields of stream 0 of the winning record "": after the first "key", the next ':', blanks, an optional
 *             '-' and decimal digits.  No header record, no dimension_count, a dimension_count outside 1 .. 2^31 - 1,
 *             a quantization outside {4, 8, 16, 32, 64} or a distance_method outside the int range: SZG_E_FORMAT
 *             (values are range-checked before they are narrowed).  Defaults: quantization 64, distance_method 0;
 *             a distance_method other than 0 and 1 is reported as read, and szg_index_create refuses it.
 *   rows      the records whose id is numeric as a search sees it, strconv.ParseUint(id, 10, 64) (collection.go:675):
 *             ASCII digits only, at least one, value < 2^64 -- no sign, blank, "0x" or embedded NUL; "007" and "7" are
 *             two records with the document id 7 -- and whose stream 1 has at least row_bytes bytes, of which the
 *             first row_bytes are the vector.  (Listing mode's id rule, collection.go:637, is not restated.)
 * No C++ exception leaves a szg_pager_* function: a failed allocation is SZG_E_NOMEM, anything else SZG_E_DEVICE.
 *
 * The Go binding does not need this (it has the spanfile in memory); it is the
 * first "next" row of SURVEY.md 8f: C/C++/Python hosts and the GPU box can open
 * real collection files.  Pure host code, no device work.
 */
#ifndef SYZGY_PAGER_H
#define SYZGY_PAGER_H

#include <stdint.h>
#include "syzgy_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct szg_pager szg_pager;

#define SZG_E_IO (-8)      /* cannot open / map the file */
#define SZG_E_FORMAT (-9)  /* no usable header record / a header value out of range */

/* Open and scan a collection file (read-only mmap). n_threads <= 0: one per core (CRC pass). */
int szg_pager_open(szg_pager **out, const char *path, int n_threads);
void szg_pager_close(szg_pager *p);

/* CollectionOptions of the header record (collection.go:31-48). */
int szg_pager_options(const szg_pager *p, int *dim, int *quant_bits, int *metric);

/* Live records with a numeric id (ParseUint's rule, above) and a vector stream of at least row_bytes bytes. */
uint64_t szg_pager_count(const szg_pager *p);
/* ACTIVE spans skipped during the scan: too short, bad checksum or malformed structure (spanfile.go:313-327). */
uint64_t szg_pager_skipped(const szg_pager *p);

/* Document ids in visit order (row r -> ids[r]). */
int szg_pager_ids(const szg_pager *p, uint64_t *ids);
/* count x row_bytes packed vectors in visit order, reference element encoding. */
int szg_pager_vectors(const szg_pager *p, uint8_t *out, uint64_t capacity_bytes);
/* Metadata (stream 0) of row r: pointer into the mapping, valid until close. */
int szg_pager_metadata(const szg_pager *p, uint64_t row, const uint8_t **data, uint64_t *len);

/* Page every vector into a scan handle created with the same options (= szg_index_load). */
int szg_pager_load(const szg_pager *p, szg_index *ix);

#ifdef __cplusplus
}
#endif
#endif
