"""Inputs for the index-build tests (tests/test_build_gen_cpu.py, tests/test_gpu_index_build.py): small alignment sets,
each sitting on one edge of impg_amd/csrc/index_build_device.hip, with the arithmetic of the edge in its docstring; a
pure-Python CIGAR tokenizer and PAF reader; and the tokenizer's own texts.

Nothing here imports the library.  tokenize() is written from the reference (parse_cigar_to_delta, impg.rs:2935-2950:
`len = len * 10 + digit` in wrapping 32-bit arithmetic, every other byte closes an op; CigarOp::new, impg.rs:81-92:
`(code << 29) | len` without a mask, any letter outside "=XIDM" is refused)."""
import numpy as np

from tests.index_ref import INT32_MAX, RECORD_DTYPE, TILE_OPS

OPS = "=XIDM"
SEQ_LEN = 10_000_000


# ---- text -> ops, PAF -> records ---------------------------------------------------------------------------------------
def tokenize(text):
    """The packed ops of a CIGAR text, as Python ints.  ValueError for a byte that is neither a digit nor one of =XIDM."""
    b = text.encode() if isinstance(text, str) else bytes(text)
    out, ln = [], 0
    for c in b:
        if 48 <= c <= 57:
            ln = (ln * 10 + (c - 48)) & 0xFFFFFFFF
            continue
        code = OPS.find(chr(c))
        if code < 0:
            raise ValueError("Invalid CIGAR operation")
        out.append(((code << 29) | ln) & 0xFFFFFFFF)
        ln = 0
    return out


def cigar_text(pairs):
    return "".join("%d%s" % (l, c) for l, c in pairs)


def paf_line(q, t, qs, qe, ts, te, strand, cigar, tail=None):
    """One PAF line; cigar None: no tag.  tail: the fields from the twelfth on, replacing "cg:Z:<cigar>"."""
    f = [q, str(SEQ_LEN), str(qs), str(qe), "-" if strand else "+", t, str(SEQ_LEN), str(ts), str(te), "1", "1", "60"]
    if tail is not None:
        f += tail
    elif cigar is not None:
        f.append("cg:Z:" + cigar)
    return "\t".join(f)


def paf_records(texts, tokens=tokenize):
    """What the reference reads from PAF files (paf.rs:118-194): sequence ids in first-seen order, the query's before the
    target's; the CIGAR of the first field that starts with "cg:Z:", whichever field that is; "\\r\\n" line ends.
    Returns (records, ops, seq_len, names, file_first)."""
    names, lens, recs, pool, file_first = {}, [], [], [], []
    for text in ([texts] if isinstance(texts, str) else texts):
        file_first.append(len(recs))
        for line in text.split("\n"):
            if line.endswith("\r"):
                line = line[:-1]
            if not line:
                continue
            f = line.split("\t")
            ids = []
            for name, ln in ((f[0], f[1]), (f[5], f[6])):
                if name not in names:
                    names[name] = len(names)
                    lens.append(int(ln))
                ids.append(names[name])
            cg = next((x[5:] for x in f if x.startswith("cg:Z:")), "")
            ops = tokens(cg)
            recs.append((ids[0], ids[1], int(f[2]), int(f[3]), int(f[7]), int(f[8]), len(pool), len(ops), 1 if f[4] == "-" else 0))
            pool.extend(int(v) for v in ops)
    file_first.append(len(recs))
    return (np.array(recs, dtype=RECORD_DTYPE), np.array(pool, dtype=np.uint32), np.array(lens, dtype=np.int64), list(names),
            np.array(file_first, dtype=np.uint64))


def sums(pairs):
    return sum(l for l, c in pairs if c in "=XDM"), sum(l for l, c in pairs if c in "=XIM")


class Fixture:
    """paf: the PAF texts (one per file) or None; records / ops / seq_len: what from_records takes (for a PAF fixture: what
    paf_records reads from the text, so both entry points see one input)."""

    def __init__(self, name, doc, bidirectional=True, paf=None, records=None, ops=None, seq_len=None, big=False):
        self.name, self.doc, self.bidirectional, self.paf, self.big = name, doc, bidirectional, paf, big
        if paf is not None:
            self.records, self.ops, self.seq_len, self.names, self.file_first = paf_records(paf)
        else:
            self.records = np.array(records, dtype=RECORD_DTYPE)
            self.ops = np.array(ops, dtype=np.uint32)
            self.seq_len = np.array(seq_len, dtype=np.int64)

    def monotone(self):
        end = 0
        for r in self.records:
            if r["cigar_off"] < end:
                return False
            end = int(r["cigar_off"]) + int(r["cigar_len"])
        return True


def _alignments_paf(alns):
    """alns: (query name, target name, query start, target start, strand, [(len, op)]); ends follow from the CIGAR."""
    lines = []
    for q, t, qs, ts, strand, pairs in alns:
        td, qd = sums(pairs)
        lines.append(paf_line(q, t, qs, qs + qd, ts, ts + td, strand, cigar_text(pairs)))
    return "\n".join(lines) + "\n"


# ---- tile fill ---------------------------------------------------------------------------------------------------------
TILE_FILL_COUNTS = (0, 1, 5, 6, 7, 13, 14, 15, 21, 22, 23, 25, 26, 27, 51, 52, 53, 78, 207, 208, 209, 235)


def _fill_ops(n, salt):
    """n ops of mixed letters and small lengths; zero-length ops at slot 0 and slot 25 of tile 0 and, from 52 ops on, all
    through tile 1."""
    out = []
    for k in range(n):
        c = OPS[(k * 7 + salt) % 5] if (k + salt) % 3 else "="
        ln = 1 + (k * 13 + salt * 5) % 37
        if k in (0, 25) or (n >= 52 and 26 <= k < 52):
            ln = 0
        out.append((ln, c))
    return out


def tile_fill():
    """tiles_kernel's `cnt = min(TILE_OPS, n - k0)`, the sub-tile sums `6u < cnt`, `14u < cnt`, `22u < cnt` (:108-111),
    `last = hb + 5 + max(cnt, 1)` (:92) and entries_kernel's `m <= INLINE_TILES` (:215).  One record per op count of
    TILE_FILL_COUNTS, per strand, forward-only (query == target) and with a reversed entry: 0 ops is no tile and seven
    0x7FFFFFFF checkpoints; 6 / 14 / 22 end a sub-tile, 7 / 15 / 23 begin the next; 26, 52, 78, 208 fill their last tile
    and 27, 53, 209 open one with a single op; 1, 3, 9 tiles leave the wave's second half idle on the last step and 2, 8
    do not; 208 ops are 8 tiles (inline checkpoints), 209 are 9 (external), so the four forms swapped x flipped occur
    both ways.  Zero-length ops sit at slots 0 and 25 and fill tile 1 of every record of 52 ops or more."""
    alns = []
    for i, n in enumerate(TILE_FILL_COUNTS):
        for strand in (0, 1):
            for fwd_only in (True, False):
                salt = i * 4 + strand * 2 + fwd_only
                t = "t%d" % (i % 3)
                alns.append((t if fwd_only else "q%d" % (i % 2), t, 1000 * i + 17 * salt, 2000 * i + 5 * salt, strand, _fill_ops(n, salt)))
    return Fixture("tile_fill", tile_fill.__doc__, paf=[_alignments_paf(alns)])


# ---- width -------------------------------------------------------------------------------------------------------------
WIDTH_SUMS = (65534, 65535, 65536)
WIDTH_WAYS = ("single", "last", "at9", "at18")


def _width_tile(total, way, letter):
    """26 ops of `letter` summing to `total`: in one op; only with the last op (the 25 before it sum to 25); with op 8,
    so that the entry before op 9 is the first to hold it (ops 9..25 have length 0); with op 17, for the entry before op 18."""
    if way == "single":
        return [(total, letter)]
    big = {"last": 25, "at9": 8, "at18": 17}[way]
    return [(1, letter) if k < big else (total - big, letter) if k == big else (0, letter) for k in range(TILE_OPS)]


def width():
    """tiles_kernel's `wide`, `pwide` (:98-100) and `lwide` (:116): tiles whose target sum alone ('D' ops) or query sum
    alone ('I' ops) is 65534, 65535 or 65536.  65534: no line is wide.  65535: the op line is (>= 0xFFFF), the prefix line
    is not (> 0xFFFF).  65536: both.  The sum arrives in a single op; only with the last op (every entry before op 25
    holds 25, so `endT - t0` alone sets pwide); before op 9 and before op 18 (the entries copied to words 2 and 3).
    Every such tile is tile 0 of one record (first half of the wave, a narrow tile beside it in the second half) and tile 1
    of another (the other way round): `wmask >> hb` must not leak across the halves."""
    alns = []
    narrow = [(3, "="), (2, "X"), (1, "I"), (1, "D")] * 6 + [(4, "="), (5, "M")]
    k = 0
    for letter in "DI":
        for total in WIDTH_SUMS:
            for way in WIDTH_WAYS:
                tile = _width_tile(total, way, letter)
                if way == "single":
                    tile = tile + [(0, "=")] * 25  # (a full tile, so that the record's next op opens tile 1)
                for first in (True, False):
                    pairs = tile + narrow if first else narrow + tile
                    alns.append(("q%d" % (k % 2), "t%d" % (k % 3), 100 + k, 300 + 2 * k, k % 2, pairs))
                    k += 1
    return Fixture("width", width.__doc__, paf=[_alignments_paf(alns)])


# ---- gap mask ----------------------------------------------------------------------------------------------------------
def gap_mask():
    """tiles_kernel's `gapmask = (ballot(on && dG) >> (hb + 6)) & 0x3FFFFFF` (:128) and identity_lines_kernel's twin
    (:638): 'I' / 'D' at slots 0, 5, 6 and 25 of tile 0 (first half of the wave) and of tile 1 (second half) is mask
    0x2000061 in both; tile 2 is 26 gap ops, mask 0x3FFFFFF; tile 3, alone on its step, has 'D' at slot 0 only."""
    spots = [(2, "ID"[k % 2]) if k in (0, 5, 6, 25) else (3 + k % 4, "=X"[k % 2]) for k in range(TILE_OPS)]
    pairs = spots + spots + [(1 + k % 3, "ID"[k % 2]) for k in range(TILE_OPS)] + [(7, "D"), (9, "=")]
    alns = [("a", "b", 10, 20, 0, pairs), ("a", "b", 500, 700, 1, pairs), ("b", "b", 5, 9000, 1, pairs)]
    return Fixture("gap_mask", gap_mask.__doc__, paf=[_alignments_paf(alns)])


# ---- order -------------------------------------------------------------------------------------------------------------
def order_paf():
    """entry_keys_kernel's key `target << 32 | start ^ 0x80000000` (:164, :169) and the stable sort behind it: on target
    B two forward entries start at 100 (records 0, 2), and the reversed entry of record 3 (query B at 100) ties with them;
    record order decides: 0, 2, 3.  Record 4 starts at 100 on both axes: its pair lands in two segments (A and B), the
    reversed one behind record 3's.  Record 1 sorts before all of them though it comes second."""
    eq = [(50, "=")]
    alns = [("A", "B", 7, 100, 0, eq), ("A", "B", 9, 40, 1, eq), ("C", "B", 11, 100, 1, eq), ("B", "C", 100, 300, 0, eq),
            ("B", "A", 100, 100, 1, eq), ("C", "C", 5, 5, 0, eq)]
    return Fixture("order_paf", order_paf.__doc__, paf=[_alignments_paf(alns)])


def _rec(q, t, qs, qe, ts, te, strand, pool, pairs):
    ops = [(OPS.index(c) << 29) | l for l, c in pairs]
    r = (q, t, qs, qe, ts, te, len(pool), len(ops), strand)
    pool.extend(ops)
    return r


def order_records():
    """The same key at its signed ends, through from_records (PAF coordinates are unsigned): starts of -5, 0 and INT32_MAX
    on target 1 must sort -5 < 0 < INT32_MAX (without `^ 0x80000000` the negative start sorts last).  `ends_t` (:226):
    te < ts and te == ts give INT32_MIN.  The running maximum (:227, `segment << 32 | te ^ 0x80000000`) must restart: the
    last entry of target 1 ends at INT32_MAX and every end on target 3 is negative.  Sequences 0, 2 and 4 own no entry:
    an empty segment first, between the others and last."""
    pool, eq = [], [(10, "=")]
    recs = [_rec(3, 1, -90, -80, INT32_MAX, INT32_MAX, 0, pool, eq),   # target 1, start INT32_MAX, te == ts
            _rec(3, 1, -70, -60, 0, 10, 1, pool, eq),
            _rec(3, 1, -50, -40, -5, 5, 0, pool, eq),
            _rec(3, 1, -30, -35, 20, 12, 1, pool, eq),                 # te < ts on both axes
            _rec(3, 1, -20, -10, 0, INT32_MAX, 0, pool, eq),           # ties with the second record at 0
            _rec(1, 1, 0, 10, 7, 17, 0, pool, eq)]                     # forward only
    return Fixture("order_records", order_records.__doc__, records=recs, ops=pool, seq_len=[SEQ_LEN] * 5)


def order_nseq(n_seq):
    """launch_sort_pairs sorts `32 + bits_for(n_seq)` key bits (:469): n_seq of 1, 2, 3 and 5 is 1, 1, 2 and 3 target
    bits.  Every sequence is a target and a query, the highest id included, with starts descending in record order."""
    pool, recs = [], []
    for k in range(3 * n_seq):
        t = (n_seq - 1 - k) % n_seq
        q = (t + 1 + k // n_seq) % n_seq
        recs.append(_rec(q, t, 1000 - 10 * k, 1012 - 10 * k, 5000 - 100 * k, 5012 - 100 * k, k % 2, pool, [(5, "="), (2, "X"), (5, "M")]))
    return Fixture("order_nseq%d" % n_seq, order_nseq.__doc__, records=recs, ops=pool, seq_len=[SEQ_LEN] * n_seq)


# ---- levels ------------------------------------------------------------------------------------------------------------
def _level_fixture(name, doc, sizes, big=False):
    rng = np.random.default_rng(len(sizes) * 1000 + sum(sizes) % 997)
    n = sum(sizes)
    rec = np.zeros(n, dtype=RECORD_DTYPE)
    rec["target_id"] = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    rec["query_id"] = len(sizes)  # a sequence that owns no entry (bidirectional=False)
    rec["target_start"] = rng.integers(0, max(8, n // 3), n)  # (many ties)
    rec["target_end"] = rec["target_start"] + rng.integers(1, 5000, n)
    rec["query_start"] = np.arange(n)
    rec["query_end"] = np.arange(n) + 10
    rec["cigar_off"] = np.arange(n)
    rec["cigar_len"] = 1
    rec["strand"] = np.arange(n) % 2
    return Fixture(name, doc, bidirectional=False, records=rec, ops=np.full(n, 10, dtype=np.uint32), seq_len=[SEQ_LEN] * (len(sizes) + 1), big=big)


def levels():
    """The segment table's `while (c > 64)` (:508) and levels_kernel's `min(pn, 64 (j + 1)) - 1` (:242): segments of 1, 64,
    65, 4096 and 4097 entries have 0, 0, 1, 1 and 2 levels.  65 = 64 + 1 and 4097 = 64^2 + 1: the last 64-block of level 1
    (and for 4097 of level 2) holds one element, so the unclamped index 64 (j + 1) - 1 reads past the segment."""
    return _level_fixture("levels", levels.__doc__, (1, 64, 65, 4096, 4097))


def level3():
    """The same at nlev = 3: 262145 = 64^3 + 1 entries on one target, levels of 4097, 65 and 2 elements, each with a
    last block of one.  Only seg, the columns and the levels are compared with the model (lines: host against device)."""
    return _level_fixture("level3", level3.__doc__, (262145,), big=True)


# ---- pool shapes for from_records ----------------------------------------------------------------------------------------
def _pool_alns():
    out = []
    for k, n in enumerate((3, 27, 1, 60, 26, 9)):
        pairs = [(1 + (k + j) % 9, OPS[(k + 2 * j) % 5]) for j in range(n)]
        td, qd = sums(pairs)
        out.append((k % 3, (k + 1) % 3 if k != 4 else k % 3, 100 * k, 100 * k + qd, 40 * k, 40 * k + td, k % 2, pairs))
    return out


def pool(shape):
    """build_index_device's op upload (:425-446): `cigar_off - ops_first` with ops_first = the batch's first op.
    in_order: the pool in record order (the batched path).  gaps: 5 unused ops (of code 5: never read) before, between
    and behind the records' CIGARs, so every batch's `lo` differs from its first record's index sum.  shared: records 1 and
    3 name the same ops (cigar_off goes back: not monotone, the pool is uploaded whole, ops_first = 0).  reversed: the
    pool laid out in reverse record order (not monotone either)."""
    alns = _pool_alns()
    pool_, recs = [], []
    bad = [5 << 29 | 1] * 5
    if shape == "reversed":
        offs = {}
        for k in reversed(range(len(alns))):
            offs[k] = len(pool_)
            pool_.extend((OPS.index(c) << 29) | l for l, c in alns[k][7])
        recs = [a[:6] + (offs[k], len(a[7]), a[6]) for k, a in enumerate(alns)]
    else:
        for k, a in enumerate(alns):
            if shape == "gaps":
                pool_.extend(bad)
            if shape == "shared" and k == 3:
                recs.append(a[:2] + (a[2], a[2] + sums(alns[1][7])[1], a[4], a[4] + sums(alns[1][7])[0]) + (recs[1][6], recs[1][7], a[6]))
                continue
            recs.append(_rec(*a[:7], pool_, a[7]))
        if shape == "gaps":
            pool_.extend(bad)
    return Fixture("pool_" + shape, pool.__doc__, records=recs, ops=pool_, seq_len=[SEQ_LEN] * 3)


def pool_bad_op():
    """tiles_kernel's `if (code > 4u) *bad_op = 1u` (:81): op 30 of record 3 (tile 1, slot 4) has code 5."""
    f = pool("in_order")
    f.name, f.doc = "pool_bad_op", pool_bad_op.__doc__
    f.ops = f.ops.copy()
    f.ops[int(f.records[3]["cigar_off"]) + 30] = (5 << 29) | 3
    return f


# ---- tokenizer texts -----------------------------------------------------------------------------------------------------
def _letter_at(byte):
    """a CIGAR whose LAST letter is byte `byte` (0-based): "1=" pairs, then a number that fills up to it"""
    head = "1=" * ((byte - 3) // 2)
    return head + "7" * (byte - len(head)) + "X"


LENGTHS = (536870911, 536870912, 536870913, 1073741825, 2147483648, 4294967295, 4294967296, 4294967301, 99999999999)
TOKEN_TEXTS = {
    # cigar_tokens_kernel walks 64 bytes a step (:294): a letter at the last byte of step 0 and at the first of step 1
    "letter_at_63": _letter_at(63) + "4=",
    "letter_at_64": _letter_at(64) + "4=",
    # the backward scan `while (st > 0 && is_digit(s[st - 1]))` (:302) crosses the step boundary: digits at bytes 60..66
    "digits_60_66": "1=" * 30 + "1234567=" + "3I",
    # 64 and 65 letters without digits: every lane of a step emits, `done` carries 64 into step 1
    "letters_64": "=" * 64,
    "letters_65": "=" * 65,
    # a digit run longer than a step: the scan walks back over 70 bytes to the record's start
    "zeros_70": "0" * 70 + "9I",
    "mixed_69": "1=" * 31 + "123456=",
    # digits after the last letter are dropped, within a step and across one
    "trailing_digits": "5=3X12",
    "trailing_digits_across": "1=" * 31 + "12345",
    "empty": "",
    "digits_only": "5",
    "letter_only": "M",
    "zero_len": "0=",
}
for _k, _v in enumerate(LENGTHS):  # (code << 29) | len without a mask: a length >= 2^29 changes the code (:306)
    TOKEN_TEXTS["len_%d" % _v] = "3=%d%s2D" % (_v, "===X===X="[_k])
CODE5_TEXT = "2684354560="  # 0xA0000000: code 5 after the OR; refused at build ("Invalid CIGAR operation")
BAD_BYTES = "Nx *"
# texts that tokenize but hold a code above 4: 0xA0000000 and 0xFFFFFFFF (code 7)
REFUSED_AT_BUILD = (CODE5_TEXT, TOKEN_TEXTS["len_4294967295"])


def bad_texts():
    """(name, CIGAR): a byte that is no digit and none of =XIDM at byte 0, 63, 64 and last (cigar_count_kernel :279)."""
    out = []
    base = "1=" * 40  # 80 bytes
    for c in BAD_BYTES:
        for pos in (0, 63, 64, len(base) - 1):
            out.append(("bad_%r_at_%d" % (c, pos), base[:pos] + c + base[pos + 1:]))
    return out


def token_paf():
    """Every text of TOKEN_TEXTS as one record; a record without any cg:Z: tag between two that have one; two cg:Z:
    fields (the first wins); the tag in the tenth field, before the twelfth; a "\\r\\n" line end; two files."""
    lines, k = [], 0
    for name, cg in TOKEN_TEXTS.items():
        if any(v >> 29 > 4 for v in tokenize(cg)):
            continue  # (refused at build: REFUSED_AT_BUILD)
        lines.append(paf_line("q%d" % (k % 3), "t%d" % (k % 2), 10 * k, 10 * k + 50, 20 * k, 20 * k + 60, k % 2, cg))
        k += 1
        if name == "letters_64":
            lines.append(paf_line("q0", "t1", 1, 2, 3, 4, 0, None))
    lines.append(paf_line("q1", "t0", 5, 50, 6, 60, 1, None, tail=["cg:Z:4=2I", "tp:A:P", "cg:Z:9X"]))
    f = paf_line("q2", "t1", 7, 70, 8, 80, 0, None).split("\t")
    f[9] = "cg:Z:6D1="
    lines.append("\t".join(f))
    lines.append(paf_line("q0", "t0", 9, 90, 10, 100, 1, "8=1X8=") + "\r")
    half = len(lines) // 2
    return Fixture("token_paf", token_paf.__doc__, paf=["\n".join(lines[:half]) + "\n", "\n".join(lines[half:]) + "\n"])


def bad_paf(cigar, first):
    """A three-record file whose first (or last) record carries `cigar`."""
    good = [paf_line("q0", "t0", 1, 11, 2, 12, 0, "10="), paf_line("q1", "t0", 3, 13, 4, 14, 1, "4=2X4=")]
    bad = paf_line("q0", "t1", 5, 15, 6, 16, 0, cigar)
    return "\n".join([bad] + good if first else good + [bad]) + "\n"


RECORD_2_30 = "q\t1000\t100\t111\t+\tt\t1000\t200\t210\t10\t11\t60\tcg:Z:5=1073741825=5=\n"


SMALL = {"tile_fill": tile_fill, "width": width, "gap_mask": gap_mask, "order_paf": order_paf, "order_records": order_records,
         "order_nseq1": lambda: order_nseq(1), "order_nseq2": lambda: order_nseq(2), "order_nseq3": lambda: order_nseq(3),
         "order_nseq5": lambda: order_nseq(5), "levels": levels, "pool_in_order": lambda: pool("in_order"),
         "pool_gaps": lambda: pool("gaps"), "pool_shared": lambda: pool("shared"), "pool_reversed": lambda: pool("reversed"),
         "token_paf": token_paf}
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        _CACHE[name] = level3() if name == "level3" else pool_bad_op() if name == "pool_bad_op" else SMALL[name]()
    return _CACHE[name]
