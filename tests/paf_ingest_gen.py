"""Fixtures for the streamed PAF ingest (tests/test_paf_ingest_cpu.py, tests/test_gpu_paf_ingest.py): small PAF texts that
each sit on one edge of the device parser, the containers they come in, and a restatement of the driver's piece cutting
(which bytes a read fetches, where a piece ends, what is carried, when the buffer doubles) that says what the counters
must read.  A fixture is a list of files' bytes; every fixture is at most 16 KB."""
import numpy as np

from tests import seq_ingest_gen as sg

PIECE_SIZES = (16, 48, 256, 1024, 4096, 0)  # 0: the default
DEFAULT_PIECE = 64 << 20
TAG = b"cg:Z:"
ERRORS = {"fields": "Not enough fields in PAF record", "number": "Invalid field", "no_strand": "Expected '+' or '-' for strand",
          "strand": "Invalid strand", "cigar": "Invalid CIGAR operation"}


def head(q=b"q1", ql=1000, qs=10, qe=110, strand=b"+", t=b"t1", tl=2000, ts=20, te=120, rest=(b"90", b"100")):
    """fields 0 .. 10 of a line, joined"""
    def n(v):
        return v if isinstance(v, bytes) else b"%d" % v
    return b"\t".join([q, n(ql), n(qs), n(qe), strand, t, n(tl), n(ts), n(te)] + list(rest))


def line(cigar=b"90=1X9=", mapq=b"255", eol=b"\n", **kw):
    """a line of 12 fields and the tag"""
    return head(**kw) + b"\t" + mapq + b"\t" + TAG + cigar + eol


def line_tag_at(cur, at, cigar, k):
    """a line that starts at file offset `cur` and has the 'c' of its tag at offset `at`: field 11 is the filler"""
    h = head(q=b"s%d" % (k % 7), t=b"s%d" % ((k + 3) % 7)) + b"\t"
    pad = at - (cur + len(h)) - 1
    assert pad >= 1, (cur, at)
    return h + b"f" * pad + b"\t" + TAG + cigar + b"\n"


def straddle():
    """the tag split k | 5 - k (k = 1 .. 4) by a lane's edge (a multiple of 16), a wave's (of 1024) and a block's (of 4096)"""
    out = bytearray()
    n = 0
    for m in range(1, 16):
        k = (m + m // 4) % 4 + 1
        out += line_tag_at(len(out), 1024 * m - k, b"%d=2I%dX" % (m, m + 1), n)
        n += 1
        kl = m % 4 + 1  # ... and a short line whose tag a lane's edge splits
        at = (len(out) + 80) // 16 * 16 + 16 - kl
        if at % 1024 >= 1024 - 8 or at + 40 > 1024 * (m + 1) - 70:
            continue
        out += line_tag_at(len(out), at, b"7=1D%d=" % m, n)
        n += 1
    return [bytes(out)]


def tag_splits(text):
    """{edge size: set of k} over the tags of `text`: the edge lies k bytes into the tag"""
    got = {16: set(), 1024: set(), 4096: set()}
    at = text.find(b"\t" + TAG)
    while at >= 0:
        p = at + 1
        for k in range(1, 5):
            for edge in got:
                if (p + k) % edge == 0:
                    got[edge].add(k)
        at = text.find(b"\t" + TAG, at + 1)
    return got


def forms():
    """every form of the tag and of a field the parser treats on its own; the last line has no newline"""
    L = [
        head() + b"\t255\t" + TAG + b"5=1X4=\ttp:A:P\tNM:i:1\n",                      # the tag is not the last field
        head(q=b"q2") + b"\t255\tNM:i:0\n",                                           # no tag: no ops
        head(q=b"q3") + b"\t255\t" + TAG + b"3=\t" + TAG + b"9X\n",                    # twice: the first wins
        head(q=TAG + b"4=2I") + b"\t255\n",                                           # the tag as field 0 (and so the query's name)
        head(q=b"q4") + b"\t255\tx" + TAG + b"8=\n",                                  # "xcg:Z:" inside a field: no tag
        head(q=b"q5") + b"\t255\t" + TAG + b"\n",                                     # nothing behind the tag
        head(q=b"q6") + b"\t255\t" + TAG + b"\r\n",                                   # ... and a '\r' behind it
        head(q=b"q7") + b"\t" + TAG + b"6=\n",                                        # exactly 12 fields, the tag the twelfth
        head(q=b"q8") + b"\tno_tag_in_12_fields\n",                                   # exactly 12 fields without a tag
        head(q=b"q9") + b"\t" + b"\t".join(b"f%d:i:%d" % (k, k) for k in range(9)) + b"\t" + TAG + b"2=1X\r\n",  # 20 fields before the tag
        line(q=b"q10", ql=b"+1000", qs=b"+7", qe=b"+0017", cigar=b"10="),             # numbers with '+'
        line(q=b"big", ql=3000000000, qs=2147483648, qe=4294967295, ts=2147483647, te=2147483648, cigar=b"1="),  # >= 2^31: the cast wraps
        line(q=b"huge", ql=18446744073709551617, qs=18446744073709551616 + 5, qe=36893488147419103232 + 9, cigar=b"2="),  # >= 2^64: wraps
        line(q=b"q1", ql=999, cigar=b"3="),                                           # a name with a second length: the first wins
        line(q=b"q", t=b"t", cigar=b"4="),                                            # names that are prefixes of others
        line(q=b"q12", t=b"t12", cigar=b"5="),
        line(q=b"", t=b"t1", cigar=b"6="),                                            # an empty name
        line(q=b"q13", t=b"", cigar=b"7=", eol=b"\r\n"),
        line(q=b"q14", cigar=b"12=3D4I5M6X7", strand=b"-", eol=b""),                  # digits behind the last letter are dropped; no final newline
    ]
    return [b"".join(L)]


def crlf_edge(size):
    """\\r\\n lines placed so that, read with a buffer of `size`, one read ends between a '\\r' and its '\\n' and the next
    read's last byte is a '\\n'"""
    len0 = 70 if size == 16 else 100 if size == 48 else 60
    l0 = line(q=b"a0", eol=b"\r\n")
    l0 = head(q=b"a0") + b"\t" + b"f" * (len0 - len(l0)) + b"255\t" + TAG + b"90=1X9=\r\n"
    assert len(l0) == len0
    cap = size
    while cap < len0:
        cap *= 2
    l1 = head(q=b"a1") + b"\t" + b"g" * (cap - len0 + 1 - len(line(q=b"a1", mapq=b"", eol=b"\r\n"))) + b"\t" + TAG + b"90=1X9=\r\n"
    assert len(l0) + len(l1) == cap + 1 and (l0 + l1)[cap - 1:cap + 1] == b"\r\n"
    l2 = head(q=b"a2") + b"\t" + b"h" * (len0 - 1 - len(line(q=b"a2", mapq=b"", eol=b"\r\n"))) + b"\t" + TAG + b"90=1X9=\r\n"
    assert len(l2) == len0 - 1
    return [l0 + l1 + l2 + line(q=b"a3", eol=b"\r\n") + line(q=b"a4", t=b"a0", eol=b"\r\n")]


def files():
    """three files whose names continue each other's ids, an empty file between two of them"""
    a = line(q=b"f1", t=b"f2") + line(q=b"f2", t=b"f3", cigar=b"5=")
    b = line(q=b"f3", t=b"f4", cigar=b"6=") + line(q=b"f5", t=b"f1", cigar=b"7=", eol=b"")
    c = line(q=b"f6", t=b"f2", tl=77, cigar=b"8=") + line(q=b"f4", t=b"f7", cigar=b"9=")
    return [a, b"", b, c]


def _big(n_bytes):
    rng = np.random.default_rng(5)
    out = bytearray()
    while len(out) < n_bytes:
        out += b"%d%s" % (int(rng.integers(1, 3000)), b"=XIDM"[int(rng.integers(0, 5))].to_bytes(1, "little"))
    return bytes(out)


def big_first():
    """one 8 KB CIGAR as a file's first line: the buffer grows at once (8000 bytes: the line fits 8192, so that pieces of 256,
    1024 and 4096 bytes still cut the file in two)"""
    return [line(q=b"b1", cigar=_big(8000)) + b"".join(line(q=b"b%d" % k, t=b"b1", cigar=b"%d=" % k) for k in range(2, 10))]


def big_last():
    """... and as a file's last line: it grows late"""
    return [b"".join(line(q=b"c%d" % k, cigar=b"%d=" % (k + 1)) for k in range(12)) + line(q=b"c1", t=b"c9", cigar=_big(8192))]


def error_file(kind):
    """a good file of 90 lines (about 5 KB: the bad line is in a later piece than the first at every size up to 4096), one bad
    line, two good lines"""
    bad = {"fields": head(q=b"bad") + b"\n", "number": line(q=b"bad", qs=b"12a"), "no_strand": line(q=b"bad", strand=b""),
           "strand": line(q=b"bad", strand=b"*"), "cigar": line(q=b"bad", cigar=b"5=3N2=")}[kind]
    good = b"".join(line(q=b"e%d" % (k % 5), t=b"e%d" % (k % 3 + 5), cigar=b"%d=1X" % (40 + k), rest=(b"90", b"100" + b"0" * (k % 7))) for k in range(90))
    return [good + bad + line(q=b"e1") + line(q=b"e2")]


def error_order(kind):
    """what the route reports when two checks fail: "same_line": one line with a bad head and a bad CIGAR (the head's);
    "cigar_first": a bad CIGAR two lines before a bad head (the CIGAR's -- the host route says the head's)"""
    if kind == "same_line":
        return [line() + line(q=b"bad", strand=b"*", cigar=b"5=3N") + line()], ERRORS["strand"]
    return [line() + line(q=b"bad", cigar=b"5=3N") + line() + line(q=b"bad2", qs=b"x")], ERRORS["cigar"]


FIXTURES = {"straddle": straddle, "forms": forms, "files": files, "big_first": big_first, "big_last": big_last,
            "crlf_16": lambda: crlf_edge(16), "crlf_48": lambda: crlf_edge(48), "crlf_256": lambda: crlf_edge(256),
            "crlf_1024": lambda: crlf_edge(1024), "crlf_4096": lambda: crlf_edge(4096)}
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        _CACHE[name] = FIXTURES[name]()
    return _CACHE[name]


def containers(data):
    """plain, one gzip stream, several gzip members, BGZF (tests.seq_ingest_gen)"""
    return sg.containers(data)


def write(texts, folder, stem, container="plain"):
    """the fixture's files in `container` -> their paths (the reader goes by the magic, not by the name)"""
    paths = []
    for k, t in enumerate(texts):
        paths.append(str(folder / ("%s.%d.%s.paf" % (stem, k, container))))
        with open(paths[-1], "wb") as f:
            f.write(containers(t)[container])
    return paths


def cut(texts, piece):
    """The driver's piece cutting restated: a read fills the buffer behind the carried bytes; the piece is the buffer up to its
    last '\\n', the rest is carried; a buffer without a '\\n' while the text goes on doubles (and stays doubled); the text's end
    closes the last piece.  -> dict(pieces, carried, grows, reads, grow_at): reads = per file, the offsets at which a read ended."""
    cap = piece or DEFAULT_PIECE
    out = dict(pieces=0, carried=0, grows=0, reads=[], grow_at=[])  # grow_at: the pieces begun when the buffer doubled
    begun = 0
    for t in texts:
        st = dict(at=0, ended=False)
        reads = []

        def next_piece(buf):
            nonlocal cap, begun
            while True:
                if not st["ended"]:
                    want = cap - len(buf)
                    got = t[st["at"]:st["at"] + want]
                    st["ended"] = len(got) < want
                    st["at"] += len(got)
                    reads.append(st["at"])
                    buf = buf + got
                if st["ended"]:
                    return buf, b""
                k = buf.rfind(b"\n")
                if k >= 0:
                    return buf[:k + 1], buf[k + 1:]
                cap *= 2
                out["grows"] += 1
                out["grow_at"].append(begun)
        p, tail = next_piece(b"")
        while p:
            begun += 1
            out["carried"] += len(tail)
            p, tail = next_piece(tail)
            out["pieces"] += 1
        out["reads"].append(reads)
    return out


STAT_KEYS = ("device", "pieces", "text_bytes", "lines", "carried_bytes", "buffer_grows", "pool_regrows", "unknown_names", "inflated_blocks")


def selftest(paths, piece, on_host=True, hash_bits=64, pool_ops=0, device=0):
    """impg_gpu_selftest_paf_ingest -> (dict in the model's shape, {counter: value}); raises ImpgGpuError"""
    import ctypes as C

    import impg_amd
    from impg_amd import _lib
    L = impg_amd.lib()
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    rec, ops, names, lens, ff = (C.c_void_p() for _ in range(5))
    n_rec, n_ops, names_len, n_seq = (C.c_size_t() for _ in range(4))
    stats = (C.c_uint64 * len(STAT_KEYS))()
    _lib.check(L.impg_gpu_selftest_paf_ingest(arr, len(paths), piece, 1 if on_host else 0, device, hash_bits, pool_ops, C.byref(rec), C.byref(n_rec),
                                              C.byref(ops), C.byref(n_ops), C.byref(names), C.byref(names_len), C.byref(lens), C.byref(n_seq),
                                              C.byref(ff), stats))
    try:
        r = np.frombuffer(C.string_at(rec.value, n_rec.value * _lib.RECORD_DTYPE.itemsize), dtype=_lib.RECORD_DTYPE)
        got = dict(records=[tuple(int(x[k]) for k in ("query_id", "target_id", "query_start", "query_end", "target_start", "target_end", "cigar_off",
                                                        "cigar_len", "strand")) for x in r],
                   ops=np.frombuffer(C.string_at(ops.value, n_ops.value * 4), dtype="<u4").tolist(),
                   names=C.string_at(names.value, names_len.value).split(b"\n") if n_seq.value else [],
                   lens=np.frombuffer(C.string_at(lens.value, n_seq.value * 8), dtype="<i8").tolist(),
                   file_first=np.frombuffer(C.string_at(ff.value, (len(paths) + 1) * 8), dtype="<u8").tolist())
    finally:
        for p in (rec, ops, names, lens, ff):
            _lib.free(p)
    return got, dict(zip(STAT_KEYS, [int(v) for v in stats]))
