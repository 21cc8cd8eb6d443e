"""Test-side MODEL of the pager's read rules (include/syzgy_pager.h), beside the writer
(spanfile_writer.py): plain Python over unbounded integers, so no sum in it can wrap.
It restates the reference's scan (spanfile.go:282-357 walk, :730-818 parseSpan, :627-636
read7Code, collection.go:241-252 header record, :674-678 the id rule of a search) with the
pager's documented deviations, and is what tests/test_pager_malformed_cpu.py holds the C++
against, line by line.

scan(blob) -> (rc_class, dim, bits, metric, skipped, [(id, metadata, vector)]) in visit order;
scan_ex(blob) also returns what the fuzz generator is tuned by (never the pager's own counts).
"""
import re
import struct
import zlib

ACTIVE = 0x5350414E
MIN_SPAN = 15
OK, IO, FORMAT = "OK", "IO", "FORMAT"
RC_OF = {OK: 0, IO: -8, FORMAT: -9}      # SZG_OK, SZG_E_IO, SZG_E_FORMAT
E_INVALID, E_RANGE = -1, -6
WIDTHS = (4, 8, 16, 32, 64)
U64 = 1 << 64
_DIGITS = re.compile(rb"[0-9]+\Z")


def row_bytes(bits, dim):
    return (dim + 1) // 2 if bits == 4 else dim * bits // 8


def read7(d, at):
    """read7Code: MSB-first base 128 in uint64 arithmetic (the value modulo 2^64).
    -> (value, next offset), or None when the continuation bits run to the span end."""
    r = 0
    for o in range(at, len(d)):
        r = ((r << 7) | (d[o] & 0x7F)) % U64
        if not d[o] & 0x80:
            return r, o + 1
    return None


def parse_span(d, stats=None):
    """Structure of a CRC-valid ACTIVE span of len(d) >= 15 bytes.
    -> (sequence, id bytes, [stream bytes by position]) or None (rejected)."""
    n = len(d)

    def big(v):
        if stats is not None and v >= 1 << 63:
            stats["huge_lengths"] += 1

    got = read7(d, 8)
    if got is None:
        return None
    seq, at = got
    got = read7(d, at)
    if got is None:
        return None
    idlen, at = got
    big(idlen)
    if at + idlen > n:                      # true arithmetic: nothing wraps here
        return None
    rid = bytes(d[at:at + idlen])
    at += idlen
    if at >= n:                             # no stream-count byte
        return None
    count = d[at]
    at += 1
    streams = []
    for _ in range(count):
        if at >= n:                         # no stream-id byte
            return None
        at += 1
        got = read7(d, at)
        if got is None:
            return None
        sl, at = got
        big(sl)
        if at + sl > n:
            return None
        streams.append(bytes(d[at:at + sl]))
        at += sl
    if at + 4 > n:                          # the trailer's 4 bytes
        return None
    return seq % (1 << 32), rid, streams


def json_int(js, key):
    """The pager's header-field rule: after the first '"key"', the next ':', blanks and tabs,
    an optional '-', then decimal digits (at least one).  -> int, or None (field absent)."""
    k = b'"' + key + b'"'
    p = js.find(k)
    if p < 0:
        return None
    p = js.find(b":", p + len(k))
    if p < 0:
        return None
    m = re.match(rb"[ \t]*(-?[0-9]+)", js[p + 1:])
    return int(m.group(1)) if m else None


def scan_ex(blob):
    stats = {"crc_valid_rejected": 0, "huge_lengths": 0, "spans": 0}
    blob = bytes(blob)
    size = len(blob)
    if size == 0:
        return (IO, 0, 0, 0, 0, []), stats
    skipped = 0
    index = {}                              # id bytes -> (sequence, streams)
    off = 0
    while off < size:
        if off + MIN_SPAN > size:
            break
        magic, length = struct.unpack_from(">II", blob, off)
        if magic == 0:
            break
        if off + length > size:
            break
        if length == 0:
            break                           # deviation: the reference refuses the file
        if magic == ACTIVE:
            stats["spans"] += 1
            d = blob[off:off + length]
            if length < MIN_SPAN:
                skipped += 1
            elif zlib.crc32(d[:-4]) & 0xFFFFFFFF != struct.unpack(">I", d[-4:])[0]:
                skipped += 1
            else:
                ps = parse_span(d, stats)
                if ps is None:
                    skipped += 1
                    stats["crc_valid_rejected"] += 1
                else:
                    seq, rid, streams = ps
                    if rid not in index or seq > index[rid][0]:
                        index[rid] = (seq, streams)
        off += length
    hdr = index.get(b"")
    js = hdr[1][0] if hdr and hdr[1] else None
    dim = json_int(js, b"dimension_count") if js is not None else None
    if dim is None:
        return (FORMAT, 0, 0, 0, skipped, []), stats
    bits = json_int(js, b"quantization")
    bits = 64 if bits is None else bits
    metric = json_int(js, b"distance_method")
    metric = 0 if metric is None else metric
    if not 1 <= dim <= 2**31 - 1 or bits not in WIDTHS or not -2**31 <= metric <= 2**31 - 1:
        return (FORMAT, 0, 0, 0, skipped, []), stats
    rb = row_bytes(bits, dim)
    rows = []
    for rid in sorted(index):               # bytes sort bytewise = sort.Strings
        if not _DIGITS.match(rid) or int(rid) >= U64:     # strconv.ParseUint(id, 10, 64)
            continue
        streams = index[rid][1]
        if len(streams) < 2 or len(streams[1]) < rb:
            continue
        rows.append((int(rid), streams[0], streams[1][:rb]))
    return (OK, dim, bits, metric, skipped, rows), stats


def scan(blob):
    return scan_ex(blob)[0]


def line(result):
    """The one line the dumpers (tests/cpp/test_pager.cpp, the SpanfilePager child) print for an open."""
    rc, dim, bits, metric, skipped, rows = result
    if rc != OK:
        return "rc=%d" % RC_OF[rc]
    need = len(rows) * row_bytes(bits, dim)
    vec = zlib.crc32(b"".join(r[2] for r in rows)) & 0xFFFFFFFF
    return ("rc=0 dim=%d bits=%d metric=%d count=%d skipped=%d short=%s range=%d ids=%s vec=%08x meta=%s"
            % (dim, bits, metric, len(rows), skipped, E_INVALID if need else "na", E_RANGE,
               ",".join(str(r[0]) for r in rows), vec,
               ",".join("%d:%08x" % (len(r[1]), zlib.crc32(r[1]) & 0xFFFFFFFF) for r in rows)))
