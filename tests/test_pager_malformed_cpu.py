"""Malformed collection files against the model of the read rules (tests/spanfile_model.py).

The pager (syzgydb_amd/csrc/spanfile_pager.cpp) is the one part of the library that reads bytes it did not write.  Here
it gets files whose spans have a correct checksum and a broken structure, lengths that wrap a 64-bit sum, cut files,
header values out of range and record ids that strconv.ParseUint refuses -- directed cases, one named file each, and a
seeded mutation fuzz -- and two runners compare what it makes of every file, line by line, with the model:
  * tests/cpp/test_pager.cpp: the pager compiled alone under -fsanitize=address,undefined, its own main;
  * the built library through SpanfilePager, in a child Python process (an abort fails one test, not the run).
Pure host code: no GPU.
"""
import os
import shutil
import struct
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

import spanfile_model as sm
import spanfile_writer as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 1 << 64
N_FUZZ = 6400


# ---------------------------------------------------------------- builders --------------------------------------------
c7, raw, all_high_trailer = sw.code7, sw.raw_span, sw.span_ending_in_a_code    # the raw-body builders


def hdr(seq, js):
    return sw.span(seq, "", [(0, js)])


def js_of(dim, bits=None, metric=None):
    s = '{"name":"t"'
    if metric is not None:
        s += ',"distance_method":%d' % metric
    s += ',"dimension_count":%d' % dim
    if bits is not None:
        s += ',"quantization":%d' % bits
    return (s + "}").encode()


DIM, BITS = 3, 8          # the directed cases' collection: 3 bytes a row
RB = 3


def vec_of(i):
    return bytes([(7 * i + 1) & 0xFF, (7 * i + 2) & 0xFF, (7 * i + 3) & 0xFF])


def good(seq, rid, i=None, meta=None):
    i = seq if i is None else i
    return sw.span(seq, rid, [(0, b"m%d" % i if meta is None else meta), (1, vec_of(i))])


def file_of(spans, header=True, tail=32):
    blob = sw.span(0, "", [], magic=sw.FREE)
    if header:
        blob += hdr(1, js_of(DIM, BITS, 1))
    return blob + b"".join(spans) + b"\x00" * tail


def directed_cases():
    """-> [(name, blob, expect)]: expect = None (the model alone decides) or (ids, skipped) / an rc class, stated by
    hand from the rules of the issue so that the model is itself held to something."""
    cases = []

    def add(name, blob, expect=None):
        cases.append((name, bytes(blob), expect))

    A, B = good(20, "41"), good(21, "42")
    two_streams = lambda v: b"\x02" + b"\x00" + c7(2) + b"mm" + b"\x01" + c7(len(v)) + v

    # --- id length -------------------------------------------------------------------------------------------------
    # after the 1-byte sequence code and a 10-byte id-length code the id starts at 8 + 1 + 10 = 19
    at = 19
    tail = b"9" + two_streams(vec_of(1))
    add("idlen_2p64m1", file_of([raw(c7(5) + c7(U64 - 1, 10) + tail), A]), ([41], 1))
    add("idlen_2p64_minus_at", file_of([raw(c7(5) + c7(U64 - at, 10) + tail), A]), ([41], 1))
    for k in (1, 2, 5):
        add("idlen_2p64_minus_at_plus_%d" % k, file_of([raw(c7(5) + c7(U64 - at + k, 10) + tail), A]), ([41], 1))
    add("idlen_2p63", file_of([raw(c7(5) + c7(1 << 63, 10) + tail), A]), ([41], 1))
    # a span of 8 + 1 + 1 + R + 4 bytes: the id starts at 10, R = 8 bytes lie between it and the trailer
    R = 8
    for name, idlen, fill, expect in (
            ("idlen_to_span_end", R + 4, b"1234567\x00", ([41], 1)),
            ("idlen_1_into_trailer", R + 1, b"1234567\x00", ([41], 1)),
            ("idlen_to_trailer", R, b"12345678", ([41], 1)),             # the count byte would be the trailer's first
            ("idlen_1_before_trailer_count0", R - 1, b"1234567\x00", ([41], 0)),   # id "1234567", no streams: accepted, no row
            ("idlen_1_before_trailer_count1", R - 1, b"1234567\x01", ([41], 1))):  # one stream counted, none there
        add(name, file_of([raw(c7(5) + c7(idlen) + fill), A]), expect)

    # --- stream length ---------------------------------------------------------------------------------------------
    for which in (0, 1):
        # seq(1) idlen(1) id(1) count(1) [sid len(1) "mm"] sid -> the 10-byte length code, then the stream
        at = 8 + 4 + (4 if which else 0) + 1 + 10
        pre = c7(5) + c7(1) + b"9" + b"\x02" + (b"\x00" + c7(2) + b"mm" + b"\x01" if which else b"\x00")
        post = vec_of(2) + (b"" if which else b"\x01" + c7(RB) + vec_of(2))
        add("streamlen%d_2p64m1" % which, file_of([raw(pre + c7(U64 - 1, 10) + post), A]), ([41], 1))
        for k in (0, 1, 2, 3):
            add("streamlen%d_wrap_plus_%d" % (which, k), file_of([raw(pre + c7(U64 - at + k, 10) + post), A]), ([41], 1))
        # the same value one 2^64 higher: an 11-byte code whose top bits shift out of the reference's uint64
        add("streamlen%d_modulo" % which, file_of([raw(pre + c7(U64 + (RB if which else 3), 11) + post), A]),
            ([41, 9], 0) if which else None)

    # --- a 7-code of continuation bytes to the span end, in each position --------------------------------------------
    add("code_runs_out_seq", file_of([all_high_trailer(b""), A]), ([41], 1))
    add("code_runs_out_idlen", file_of([all_high_trailer(c7(5)), A]), ([41], 1))
    add("code_runs_out_streamlen", file_of([all_high_trailer(c7(5) + c7(1) + b"9" + b"\x01\x00"), A]), ([41], 1))
    add("code_ends_in_trailer", file_of([raw(c7(5) + c7(1) + b"9" + b"\x01\x00" + b"\x80\x80\x80"), A]))

    # --- stream count ------------------------------------------------------------------------------------------------
    add("streams_0", file_of([sw.span(5, "9", []), A]), ([41], 0))
    add("streams_1", file_of([sw.span(5, "9", [(0, b"mm")]), A]), ([41], 0))
    add("streams_3", file_of([sw.span(5, "9", [(0, b"mm"), (1, vec_of(3)), (2, b"third")]), A]), ([41, 9], 0))
    add("streams_255_two_present", file_of([raw(c7(5) + c7(1) + b"9" + b"\xff" + two_streams(vec_of(3))[1:]), A]), ([41], 1))
    add("streams_255_two_present_padded", file_of([raw(c7(5) + c7(1) + b"9" + b"\xff" + two_streams(vec_of(3))[1:]
                                                     + b"\x00" * 40), A]))

    # --- vector stream -----------------------------------------------------------------------------------------------
    add("vector_short_by_1", file_of([sw.span(5, "9", [(0, b"mm"), (1, vec_of(3)[:RB - 1])]), A]), ([41], 0))
    add("vector_long_by_3", file_of([sw.span(5, "9", [(0, b"mm"), (1, vec_of(3) + b"xyz")]), A]), ([41, 9], 0))
    add("vector_short_shadows_older", file_of([good(4, "9"), sw.span(5, "9", [(0, b"mm"), (1, b"ab")]), A]), ([41], 0))

    # --- span length field, a good record behind it --------------------------------------------------------------------
    add("length_0", file_of([A, struct.pack(">II", sw.ACTIVE, 0) + b"\x01" * 8, B]), ([41], 0))   # the walk stops: B unseen
    add("length_8", file_of([A, struct.pack(">II", sw.ACTIVE, 8), B]), ([41, 42], 1))            # B starts where it ends
    add("length_14", file_of([A, struct.pack(">II", sw.ACTIVE, 14) + b"\x01" * 6, B]), ([41, 42], 1))
    for n in (1, 7):                                                   # the walk goes on inside the span's own header
        add("length_%d" % n, file_of([A, struct.pack(">II", sw.ACTIVE, n) + b"\x01" * 8, B]))
    s = good(5, "9")
    own = len(s)
    add("length_plus_1", file_of([A, s[:4] + struct.pack(">I", own + 1) + s[8:], B]))
    add("length_minus_1", file_of([A, s[:4] + struct.pack(">I", own - 1) + s[8:], B]))
    padded = sw.span(5, "9", [(0, b"m5"), (1, vec_of(5))], pad=1)
    short = raw(padded[8:-5], length=len(padded) - 1)                  # the same record one byte shorter, CRC made again
    add("length_minus_1_crc_repaired", file_of([A, short + padded[-1:], B]))
    add("length_minus_1_crc_repaired_aligned", file_of([A, short, B]), ([41, 42, 9], 0))
    add("length_past_end", file_of([A, s[:4] + struct.pack(">I", 1 << 20) + s[8:], B]), ([41], 0))
    add("length_past_end_by_1", file_of([A, s[:4] + struct.pack(">I", own + 1) + s[8:]], tail=0), ([41], 0))
    add("length_exactly_to_end", file_of([A, s], tail=0), ([41, 9], 0))
    add("length_max_u32", file_of([A, s[:4] + struct.pack(">I", 0xFFFFFFFF) + s[8:], B]), ([41], 0))

    # --- magic -----------------------------------------------------------------------------------------------------
    add("magic_unknown", file_of([struct.pack(">I", 0x12345678) + s[4:], A]), ([41], 0))
    add("magic_free", file_of([sw.span(5, "9", [(0, b"m"), (1, vec_of(5))], magic=sw.FREE), A]), ([41], 0))
    add("magic_zero", file_of([A, b"\x00" * 4 + s[4:], B]), ([41], 0))
    add("crc_wrong", file_of([sw.span(5, "9", [(0, b"m"), (1, vec_of(5))], corrupt=True), A]), ([41], 1))

    # --- files -----------------------------------------------------------------------------------------------------
    add("file_0_bytes", b"", sm.IO)
    add("file_1_byte", b"S", sm.FORMAT)
    add("file_14_bytes", sw.span(0, "", [], magic=sw.FREE)[:14], sm.FORMAT)
    add("file_15_bytes", sw.span(0, "", [], magic=sw.FREE), sm.FORMAT)
    whole = file_of([good(7, "30"), A, B], tail=0)
    for cut in range(len(whole) - len(A) - len(B), len(whole) + 1):
        left = len(whole) - cut
        add("cut_%03d" % cut, whole[:cut], ([30, 41, 42][:1 + (left <= len(B)) + (left == 0)], 0))

    # --- header ----------------------------------------------------------------------------------------------------
    add("header_absent", file_of([A], header=False), sm.FORMAT)
    add("header_no_streams", file_of([sw.span(1, "", []), A], header=False), sm.FORMAT)
    add("header_no_dimension", file_of([hdr(1, b'{"quantization":8}'), A], header=False), sm.FORMAT)
    for dim in (0, -3, 2147483648, 4294967298, 4294967299, 1 << 63, (1 << 64) + 3, 10**30):
        add("header_dim_%d" % dim, file_of([hdr(1, js_of(dim, 8, 0)), A], header=False), sm.FORMAT)
    add("header_dim_max", file_of([hdr(1, js_of(2147483647, 64, 0)), A], header=False), ([], 0))
    for bits in (7, 0, -8, 4294967304, 128):
        add("header_quantization_%d" % bits, file_of([hdr(1, js_of(3, bits, 0)), A], header=False), sm.FORMAT)
    add("header_metric_out_of_int", file_of([hdr(1, js_of(3, 8, 4294967297)), A], header=False), sm.FORMAT)
    v8 = bytes(range(24))
    add("header_defaults", file_of([hdr(1, js_of(3)), sw.span(9, "5", [(0, b"m"), (1, v8)])], header=False))
    add("header_twice_higher_last", file_of([hdr(1, js_of(1, 16, 0)), hdr(2, js_of(DIM, BITS, 1)), A], header=False), ([41], 0))
    add("header_twice_higher_first", file_of([hdr(2, js_of(DIM, BITS, 1)), hdr(1, js_of(1, 16, 0)), A], header=False), ([41], 0))
    add("header_twice_equal_sequence", file_of([hdr(2, js_of(DIM, BITS, 1)), hdr(2, js_of(1, 16, 0)), A], header=False), ([41], 0))
    add("sequence_modulo_2p32", file_of([good(7, "9", 1), raw(c7((1 << 32) + 3) + good(3, "9", 2)[9:-4])]), ([9], 0))

    # --- ids: strconv.ParseUint(id, 10, 64) ------------------------------------------------------------------------------
    for n, rid in enumerate(("-5", " 6", "+7", "8 ", "0x9", "18446744073709551616", "7\x00", "\x007", "1e3", "٣", "1_0",
                             "99999999999999999999999999")):
        add("id_refused_%d" % n, file_of([good(5, rid), A]), ([41], 0))
    add("id_max_u64", file_of([good(5, "18446744073709551615"), A]), ([18446744073709551615, 41], 0))
    add("id_leading_zeros", file_of([good(5, "007"), good(6, "7"), good(7, "0")]), ([0, 7, 7], 0))
    return cases


def big_file():
    """One file of more than 1 024 spans (the pager's parallel pass), a tenth of them damaged in turn by every means."""
    dim, bits = 5, 16
    rng = np.random.default_rng(77)
    spans = [sw.span(0, "", [], magic=sw.FREE), hdr(1, js_of(dim, bits, 0))]
    for i in range(1150):
        v = bytes(rng.integers(0, 256, 10).astype(np.uint8))
        rid = str(int(rng.integers(0, 700)))
        s = sw.span(2 + i, rid, [(0, b"meta%d" % i), (1, v)])
        if i % 10 == 3:
            how = (i // 10) % 6
            body = s[8:-4]
            codes = code_positions(s)                   # sequence, id length, metadata length, vector length
            if how == 0:
                s = sw.span(2 + i, rid, [(0, b"meta"), (1, v)], corrupt=True)
            elif how == 1:                              # id length 2^64 - 1
                s = raw(s[8:codes[1][0]] + c7(U64 - 1, 10) + s[codes[1][1]:-4])
            elif how == 2:                              # vector length: the sum wraps to 1
                s = raw(s[8:codes[3][0]] + c7(U64 - (codes[3][0] + 10) + 1, 10) + v)
            elif how == 3:
                s = raw(body[:-3])                      # the vector stream runs into the trailer
            elif how == 4:
                s = all_high_trailer(s[8:codes[0][1]])
            else:                                       # 255 streams counted, two present
                count_at = codes[2][0] - 2
                s = raw(s[8:count_at] + b"\xff" + s[count_at + 1:-4])
        spans.append(s)
    return b"".join(spans) + b"\x00" * 100


# -------------------------------------------------------------- seeded fuzz -------------------------------------------
IDS = ["1", "2", "3", "10", "21", "007", "7", "-5", " 6", "+7", "8 ", "0x9", "18446744073709551616",
       "18446744073709551615", "abc"]


def code_positions(s):
    """Offsets (start, end) of the 7-codes of a well-formed span: sequence, id length, each stream's length."""
    out = []
    v, e = sm.read7(s, 8)
    out.append((8, e))
    idlen, e2 = sm.read7(s, e)
    out.append((e, e2))
    at = e2 + idlen
    n = s[at]
    at += 1
    for _ in range(n):
        at += 1
        sl, e = sm.read7(s, at)
        out.append((at, e))
        at = e + sl
    return out


def fuzz_file(seed):
    rng = np.random.default_rng(seed)
    ri = lambda lo, hi: int(rng.integers(lo, hi))
    dim = (1, 2, 3, 5)[ri(0, 4)]
    bits = sm.WIDTHS[ri(0, 5)]
    rb = sm.row_bytes(bits, dim)
    js = js_of(dim, bits, ri(0, 2))
    spans = [sw.span(0, "", [], magic=sw.FREE), hdr(1, js)]
    protect = {1: (spans[1].index(js), spans[1].index(js) + len(js))}     # the header's JSON bytes are left alone
    for r in range(ri(1, 7)):
        rid = IDS[ri(0, len(IDS))] if rng.random() < 0.8 else str(ri(0, 10**6))
        meta = bytes(rng.integers(0, 256, ri(0, 12)).astype(np.uint8))
        streams = [(0, meta), (1, bytes(rng.integers(0, 256, rb + (ri(-1, 3) if rng.random() < 0.1 else 0)).astype(np.uint8)))]
        if rng.random() < 0.05:
            streams = streams[:ri(0, 2)]
        spans.append(sw.span(ri(2, 40), rid, streams, pad=(0, 0, 0, 2, 9)[ri(0, 5)]))
    cut = None
    for _ in range((1, 1, 2, 3)[ri(0, 4)]):
        i = ri(2, len(spans)) if rng.random() < 0.88 else 1          # a record's span, now and then the header's
        s = bytearray(spans[i])
        kind = rng.random()
        if struct.unpack_from(">I", s, 4)[0] != len(s):               # its length is damaged already: leave that be
            kind = max(kind, 0.80)
        if kind < 0.30:                                               # body bytes, CRC repaired
            lo, hi = protect.get(i, (0, 0))
            where = [p for p in range(8, len(s) - 4) if not lo <= p < hi]
            for _ in range(ri(1, 4)):
                p = where[ri(0, len(where))]
                s[p] = (0x00, 0x7F, 0x80, 0xFF, ri(0, 256), ri(0, 256), s[p] ^ (1 << ri(0, 8)), (s[p] + 1) & 0xFF)[ri(0, 8)]
            s = bytearray(raw(bytes(s[8:-4]), magic=struct.unpack_from(">I", s)[0]))
        elif kind < 0.62:                                             # a long 7-code put in, length and CRC repaired
            try:
                codes = code_positions(bytes(s))
            except (TypeError, IndexError):
                codes = []
            if codes:
                a, e = codes[ri(0, len(codes))]
                old = sm.read7(bytes(s), a)[0]
                pick = ri(0, 8)
                at10 = a + 10
                value, width = ((U64 - 1, 10), (U64 - at10 + ri(0, 6), 10), (1 << 63, 10), ((1 << 63) + ri(0, 1 << 62), 10),
                                (old, ri(2, 10)), (old + U64 * ri(1, 100), 11), (old + ri(-2, 3) if old > 2 else old + 1, 0),
                                (len(s) - a + ri(-12, 4), 0))[pick]
                s = bytearray(raw(bytes(s[8:a]) + c7(max(value, 0), width) + bytes(s[e:-4])))
        elif kind < 0.80:                                             # the length field, with and without CRC repair
            own = len(s)
            new = (0, ri(1, 15), own - 1, own + 1, own - ri(1, 6), own + ri(1, 6), ri(0, 1 << 32), own + 4096)[ri(0, 8)]
            if rng.random() < 0.5 and 12 <= new <= own + 8:
                body = bytes(s[8:-4])
                body = body[:new - 12] if new < own else body + b"\x00" * (new - own)
                s = bytearray(raw(body, length=new) + bytes(s[new:] if new < own else b""))
            else:
                struct.pack_into(">I", s, 4, max(new, 0))
        elif kind < 0.90:                                             # the magic
            struct.pack_into(">I", s, 0, (sw.FREE, 0, ri(1, 1 << 32), sw.ACTIVE ^ (1 << ri(0, 32)))[ri(0, 4)])
        else:                                                         # a cut tail
            cut = ri(0, 40)
        spans[i] = bytes(s)
    blob = b"".join(spans) + b"\x00" * (0, 0, 15, 64)[ri(0, 4)]
    if cut is not None:
        blob = blob[:max(0, len(blob) - cut)] if rng.random() < 0.9 else blob[:ri(0, len(blob) + 1)]
    return blob


# ------------------------------------------------------------------ corpus -------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """Every file written once, with the line the model expects for it; shared by both runners."""
    t0 = time.time()
    d = tmp_path_factory.mktemp("pager_files")
    files = [(name, blob, sm.scan_ex(blob), expect) for name, blob, expect in directed_cases()]
    big = big_file()
    files.append(("big_parallel", big, sm.scan_ex(big), None))
    n_directed = len(files)
    for seed in range(N_FUZZ):
        blob = fuzz_file(1000 + seed)
        files.append(("z%04d" % seed, blob, sm.scan_ex(blob), None))
    want = {}
    for name, blob, (result, _), _ in files:
        (d / name).write_bytes(blob)
        want[name] = sm.line(result)
    return {"dir": d, "files": files, "want": want, "n_directed": n_directed, "seconds": time.time() - t0}


def check_lines(out, corpus):
    got = {}
    for ln in out.splitlines():
        name, t, rest = ln.split(" ", 2)
        got.setdefault(name, []).append((t, rest))
    wrong = []
    for name, _, _, _ in corpus["files"]:
        lines = got.get(name, [])
        if [t for t, _ in lines] != ["t=1", "t=2", "t=3"]:
            wrong.append("%s: lines %r" % (name, lines))
        wrong += ["%s %s\n  pager %s\n  model %s" % (name, t, rest, corpus["want"][name])
                  for t, rest in lines if rest != corpus["want"][name]]
    assert not wrong, "%d of %d files differ from the model:\n%s" % (len(wrong), len(corpus["files"]), "\n".join(wrong[:20]))


# ------------------------------------------------------------------- tests -------------------------------------------
def test_model_on_the_directed_cases(corpus):
    """The model is held to expectations stated by hand, case by case, before anything is held to the model."""
    stated = 0
    for name, blob, (result, stats), expect in corpus["files"][:corpus["n_directed"]]:
        if expect is None:
            continue
        stated += 1
        if isinstance(expect, str):
            assert result[0] == expect, name
        else:
            assert result[0] == sm.OK, name
            assert ([r[0] for r in result[5]], result[4]) == expect, name
    assert stated >= 100
    result, stats = corpus["files"][corpus["n_directed"] - 1][2]
    assert stats["spans"] >= 1100 and result[4] == 115 and stats["crc_valid_rejected"] >= 90
    # the modulo rule and the served rows, spelled out once
    by = {name: res for name, _, (res, _), _ in corpus["files"][:corpus["n_directed"]]}
    assert by["streamlen1_modulo"][5][1] == (9, b"mm", vec_of(2))
    assert by["vector_long_by_3"][5][1] == (9, b"mm", vec_of(3))
    assert by["header_defaults"][1:4] == (3, 64, 0) and by["header_defaults"][5] == [(5, b"m", bytes(range(24)))]
    assert by["sequence_modulo_2p32"][5] == [(9, b"m1", vec_of(1))]       # 2^32 + 3 is sequence 3: the older span stays
    assert by["id_leading_zeros"][5] == [(0, b"m7", vec_of(7)), (7, b"m5", vec_of(5)), (7, b"m6", vec_of(6))]


def test_fuzz_generator_reaches_the_rules(corpus):
    """What the mutations reach is counted by the model, never by the pager."""
    fuzz = corpus["files"][corpus["n_directed"]:]
    refused = sum(1 for _, _, (res, _), _ in fuzz if res[0] != sm.OK)
    rejected = sum(1 for _, _, (res, st), _ in fuzz if res[0] == sm.OK and st["crc_valid_rejected"])
    huge = sum(1 for _, _, (_, st), _ in fuzz if st["huge_lengths"])
    left_out = sum(1 for _, blob, (res, _), _ in fuzz if res[0] == sm.OK and res[4] == 0 and len(res[5]) == 0)
    print("fuzz files %d: refused %d, open with a CRC-valid span rejected for structure %d, with a length >= 2^63 %d, "
          "open and empty %d; corpus built in %.1f s" % (len(fuzz), refused, rejected, huge, left_out, corpus["seconds"]))
    assert len(fuzz) >= 6000
    assert refused >= 0.02 * len(fuzz)
    assert rejected >= 0.02 * len(fuzz)
    assert huge >= 20


def test_sanitizer_program_agrees_with_the_model(corpus, tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/cpp/test_pager.cpp"
    exe = str(tmp_path / "test_pager")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # (the program carries its runtimes: nothing to preload)
                    "-pthread", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_pager.cpp"),
                    os.path.join(ROOT, "syzgydb_amd", "csrc", "spanfile_pager.cpp")], check=True)
    names = [f[0] for f in corpus["files"]]
    out = ""
    t0 = time.time()
    for i in range(0, len(names), 1000):
        done = subprocess.run([exe] + names[i:i + 1000], cwd=str(corpus["dir"]), capture_output=True, text=True)
        assert done.returncode == 0, "after %s:\n%s" % (done.stdout.splitlines()[-1:] or names[i], done.stderr[-4000:])
        assert done.stderr == "", done.stderr[-4000:]
        out += done.stdout
    print("sanitizer program: %d files in %.1f s" % (len(names), time.time() - t0))
    check_lines(out, corpus)


def test_built_library_agrees_with_the_model(corpus, tmp_path):
    """SpanfilePager over the same files in a fresh child process, with the environment this one has."""
    listing = tmp_path / "files.txt"
    listing.write_text("\n".join(f[0] for f in corpus["files"]))
    t0 = time.time()
    done = subprocess.run([sys.executable, os.path.abspath(__file__), str(listing)], cwd=str(corpus["dir"]),
                          capture_output=True, text=True)
    assert done.returncode == 0, "the child ended with %d after %s:\n%s" % (
        done.returncode, done.stdout.splitlines()[-1:], done.stderr[-4000:])
    print("library child: %d files in %.1f s" % (len(corpus["files"]), time.time() - t0))
    check_lines(done.stdout, corpus)


def child_main(listing):
    """The dumper of tests/cpp/test_pager.cpp again, through the Python binding."""
    import ctypes
    sys.path.insert(0, ROOT)
    from syzgydb_amd import SpanfilePager, SzgError
    u8p = ctypes.POINTER(ctypes.c_uint8)
    for name in open(listing).read().split("\n"):
        for t in (1, 2, 3):
            try:
                pg = SpanfilePager(name, n_threads=t)
            except SzgError as e:
                print("%s t=%d rc=%d" % (name, t, e.code), flush=True)
                continue
            with pg:
                need = pg.count * pg.row_bytes
                short = "na"
                if need:
                    buf = (ctypes.c_uint8 * need)()
                    short = pg._L.szg_pager_vectors(pg._h, ctypes.cast(buf, u8p), need - 1)
                p, n = u8p(), ctypes.c_uint64(0)
                rng = pg._L.szg_pager_metadata(pg._h, pg.count, ctypes.byref(p), ctypes.byref(n))
                meta = [pg.metadata(r) for r in range(pg.count)]
                print("%s t=%d rc=0 dim=%d bits=%d metric=%d count=%d skipped=%d short=%s range=%d ids=%s vec=%08x meta=%s"
                      % (name, t, pg.dim, pg.quant_bits, pg.metric, pg.count, pg.skipped, short, rng,
                         ",".join(str(int(x)) for x in pg.ids()), zlib.crc32(pg.vectors().tobytes()) & 0xFFFFFFFF,
                         ",".join("%d:%08x" % (len(m), zlib.crc32(m) & 0xFFFFFFFF) for m in meta)), flush=True)


if __name__ == "__main__":
    child_main(sys.argv[1])
