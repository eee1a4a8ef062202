"""Generators for the tests of impg_gpu_index_load_sequences (tests/test_seq_ingest_cpu.py, tests/test_gpu_seq_ingest.py): the
edge file, the large file, the containers a sequence file comes in (one gzip stream, gzip members, BGZF written here from
raw deflate with chosen block sizes), a restatement of the piece cutting with the kinds of piece edge a text offers, and
the index that only has to know names and lengths."""
import gzip
import struct
import zlib

import numpy as np

EDGE_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 79, 80, 81, 1023, 1024, 1025]
PIECE_SIZES = [16, 32, 48, 64, 80, 112, 256, 4096]
DEFAULT_PIECE = 64 << 20
EDGE_KINDS = ("inside a name", "right after '>'", "between \\r and \\n", "between \\n and '>'", "inside a description", "inside a run",
              "on a 16-base word edge", "inside a word", "at a sequence's last base", "inside an empty line")
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_IUPAC = np.frombuffer(b"ACGTACGTACGTacgtNnRYKMSWryk", dtype=np.uint8)


def _bases(rng, n):
    return bytearray(_IUPAC[rng.integers(0, _IUPAC.size, size=n)].tobytes())


def edge_file(seed=19):
    """-> (text, [(name, bases as the file spells them)]): sequences of EDGE_LENGTHS bases; body lines of 1, 60 and 80 bases
    and unbroken ones; one record with CRLF; blank lines; a last line without a newline; descriptions after a space and after
    a tab (their lengths drawn from the seed, which moves every later byte against the piece edges); lower case, IUPAC codes
    and a '>' in mid-line; N runs at a sequence's first and last base, NNNRR, a run across base 1024, a sequence that is one
    run.  (Seed 19: the pieces of PIECE_SIZES meet every kind of EDGE_KINDS, which tests/test_seq_ingest_cpu.py asserts.)"""
    rng = np.random.default_rng(seed)
    widths = [1, 60, 80, 0]
    out, seqs = bytearray(), []
    for k, n in enumerate(EDGE_LENGTHS):
        b = _bases(rng, n)
        if n == 64:
            b[:] = b"N" * n  # a run that is the whole sequence
        if n == 65:
            b[20] = ord(">")  # a '>' that is not at a line start is a base
        if n >= 79:
            b[0:3] = b"NNN"  # a run at the first base, one at the last, two different runs side by side
            b[n - 4:] = b"nnNN"
            b[30:35] = b"NNNRR"
        if n == 1025:
            b[1000:1024] = b"A" * 24
            b[1018:1021] = b"NNN"
            b[1021:1025] = b"NNNN"  # (with the line above: one run across base 1024, up to the last base)
        name = "s%d_%d" % (k, n)
        crlf = n == 1023
        eol = b"\r\n" if crlf else b"\n"
        desc = b"" if k % 3 == 0 else (b" " if k % 3 == 1 else b"\t") + b"d" * int(rng.integers(1, 24)) + b" x=1"
        out += b">" + name.encode() + desc + eol
        w = 60 if crlf else 80 if n == 65 else widths[k % 4] if n <= 81 or widths[k % 4] != 1 else 60
        lines = [bytes(b[i:i + w]) for i in range(0, n, w)] if w else ([bytes(b)] if n else [])
        for j, line in enumerate(lines):
            out += line + eol
            if j % 7 == 3 and not crlf:
                out += b"\n"  # a blank line inside the body
        if k % 5 == 2:
            out += b"\n\n"  # ... and two between records
        seqs.append((name, bytes(b)))
    return bytes(out).rstrip(b"\n"), seqs  # the last line without its newline


def large_file(seed=1):
    """about 300 KB: one sequence of 200 000 bases in one unbroken line, 500 short ones in lines of 70, 2 % of the bytes not
    A/C/G/T (scattered singles and a few longer N runs) -> (text, [(name, bases)])"""
    rng = np.random.default_rng(seed)
    out, seqs = bytearray(), []

    def make(n):
        b = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
        hit = rng.random(n) < 0.02
        b[hit] = np.frombuffer(b"NRYn", dtype=np.uint8)[rng.integers(0, 4, size=int(hit.sum()))]
        return bytearray(b.tobytes())
    big = make(200000)
    big[70000:70500] = b"N" * 500
    big[131000:131072 + 40] = b"N" * 112
    out += b">big one line\n" + big + b"\n"
    seqs.append(("big", bytes(big)))
    for k in range(500):
        b = make(int(rng.integers(1, 400)))
        out += b">short%d\n" % k + b"".join(bytes(b[i:i + 70]) + b"\n" for i in range(0, len(b), 70))
        seqs.append(("short%d" % k, bytes(b)))
    return bytes(out), seqs


def stored(seqs):
    """what the store holds of (name, bases as spelled): upper case"""
    return [(nm, b.upper()) for nm, b in seqs]


# ---- containers -------------------------------------------------------------------------------------------------------------
def bgzf_block(data, crc=None, isize=None, bsize=None):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    total = 18 + len(body) + 8
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", (total if bsize is None else bsize + 1) - 1) + body +
            struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize))


def bgzf(data, block_sizes=(1, 100, 65280), empty_after=2, eof=True):
    """BGZF of `data`: blocks of block_sizes input bytes in turn, an empty block after block `empty_after`, the 28-byte EOF block"""
    out, at, k = bytearray(), 0, 0
    while at < len(data):
        n = block_sizes[k % len(block_sizes)]
        out += bgzf_block(data[at:at + n])
        at += n
        if k == empty_after:
            out += bgzf_block(b"")
        k += 1
    return bytes(out) + (BGZF_EOF if eof else b"")


def gzip_members(data, parts=3):
    """gzip members without a BC subfield, back to back"""
    cut = [len(data) * i // parts for i in range(parts + 1)]
    return b"".join(gzip.compress(data[a:b], mtime=0) for a, b in zip(cut, cut[1:]))


def containers(data):
    return {"plain": data, "gzip": gzip.compress(data, mtime=0), "bgzf": bgzf(data), "members": gzip_members(data)}


# ---- the piece cutting, restated --------------------------------------------------------------------------------------------
def pieces(text, size):
    return [text[i:i + size] for i in range(0, len(text), size)]


def n_pieces(texts, size):
    return sum((len(t) + size - 1) // size for t in texts)


def edge_kinds(text, size):
    """the kinds of piece edge (EDGE_KINDS) that cutting `text` into pieces of `size` meets: an edge lies between bytes c - 1 and c"""
    kinds = set()
    cuts = set(range(size, len(text), size))
    at, in_seq, idx = 0, False, 0
    prev_base = None  # (byte, is last base so far) of the previous base of the open sequence
    lines = text.split(b"\n")
    for li, line in enumerate(lines):
        end = at + len(line)  # the line's '\n' (or the text's end)
        if line.startswith(b">"):
            name_end = at + 1
            while name_end < end and text[name_end:name_end + 1] not in (b" ", b"\t", b"\r", b"\v", b"\f"):
                name_end += 1
            for c in cuts:
                if c == at + 1:
                    kinds.add("right after '>'")
                elif at + 1 < c < name_end:
                    kinds.add("inside a name")
                elif name_end < c < end:
                    kinds.add("inside a description")
            in_seq, idx, prev_base = True, 0, None
        else:
            if at in cuts and at > 0 and line == b"" and li + 1 < len(lines):
                kinds.add("inside an empty line")
            for j, ch in enumerate(line):
                c = at + j
                if ch == 13:
                    continue
                if c in cuts and prev_base is not None and j > 0 and line[j - 1] != 13:
                    kinds.add("on a 16-base word edge" if idx % 16 == 0 else "inside a word")
                    up, pup = bytes([ch]).upper(), bytes([prev_base]).upper()
                    if up == pup and up not in (b"A", b"C", b"G", b"T"):
                        kinds.add("inside a run")
                prev_base = ch
                idx += 1
        if end in cuts and end > at and text[end - 1:end] == b"\r":
            kinds.add("between \\r and \\n")
        nxt = end + 1
        if nxt in cuts and text[nxt:nxt + 1] == b">":
            kinds.add("between \\n and '>'")
        if in_seq and not line.startswith(b">") and line.rstrip(b"\r") and (end - (1 if line.endswith(b"\r") else 0)) in cuts:
            # the cut lies right behind this line's last base: the sequence's last if only blank lines follow up to the next '>'
            k = li + 1
            while k < len(lines) and lines[k].rstrip(b"\r") == b"":
                k += 1
            if k >= len(lines) or lines[k].startswith(b">"):
                kinds.add("at a sequence's last base")
        at = end + 1
    return kinds


# ---- the index and the store, for the comparison ----------------------------------------------------------------------------
def paf_of(names, lens):
    """a PAF whose index knows `names` with `lens`, ids in this order (an index only has to know names and lengths)"""
    return "".join("%s\t%d\t0\t1\t+\t%s\t%d\t0\t1\t1\t1\t60\tcg:Z:1=\n" % (q, lq, t, lt)
                   for (q, lq), (t, lt) in zip(zip(names, lens), list(zip(names, lens))[1:]))


def unpack(store, off, n, run_start, run_end, run_byte):
    """a sequence of n bases at base `off` of the packed stream, its runs laid over the letters"""
    idx = off + np.arange(n, dtype=np.int64)
    codes = (store[idx >> 2] >> (2 * (idx & 3)).astype(np.uint8)) & 3
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].copy()
    for s, e, c in zip(run_start.tolist(), run_end.tolist(), run_byte.tolist()):
        b[s:e] = c
    return b.tobytes()


# ---- files --------------------------------------------------------------------------------------------------------------------
def put(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def malformed(tmp_path):
    """name -> (files, index names, index lengths, code, words of the message); shared with the GPU test of the real call"""
    long_name = "n" * 40
    good = b">a\nACGT\n>b\nGG\n"
    raw = b">a\n" + b"ACGTACGTAC\n" * 30
    gz = gzip.compress(raw, mtime=0)
    blocks = [bgzf_block(raw[:200]), bgzf_block(raw[200:])]
    cases = {
        "duplicate within a piece": ([b">a\nAC\n>a\nGT\n"], ["a"], [2], -1, "sequence 'a' occurs twice"),
        "duplicate across pieces": ([b">" + long_name.encode() + b"\nAC\n" + b">q\n" + b"A" * 64 + b"\n>" + long_name.encode() + b" again\nGT\n"],
                                    [long_name], [2], -1, "'" + long_name + "' occurs twice"),
        "duplicate across files": ([good, b">c\nA\n>b\nGG\n"], ["a", "b"], [4, 2], -1, "sequence 'b' occurs twice"),
        "duplicate the index lacks": ([b">z\nAC\n>a\nACGT\n>z\nGT\n"], ["a"], [4], -1, "sequence 'z' occurs twice"),
        "empty name": ([b">a\nACGT\n> desc\nGG\n"], ["a"], [4], -1, "a '>' line without a name in "),
        "text before '>'": ([b"ACGT\n>a\nACGT\n"], ["a"], [4], -1, "not a FASTA file"),
        "one base longer": ([b">a\nACGT\n>b\nGGG\n"], ["a", "b"], [4, 2], -1, "sequence 'b' has 3 bases in the sequence files and 2 in the index"),
        "one base shorter": ([b">a\nACG\n>b\nGG\n"], ["a", "b"], [4, 2], -1, "sequence 'a' has 3 bases in the sequence files and 4 in the index"),
        "gzip truncated in the header": ([gz[:6]], ["a"], [300], -4, "truncated"),
        "gzip truncated in a block": ([gz[:len(gz) // 2]], ["a"], [300], -4, "Failed to decompress"),
        "gzip truncated before the trailer": ([gz[:-8]], ["a"], [300], -4, "truncated"),
        "bgzf truncated in a block": ([blocks[0] + blocks[1][:30]], ["a"], [300], -4, "BSIZE leads outside the file"),
        "bgzf truncated in the header": ([blocks[0] + blocks[1][:10]], ["a"], [300], -4, "block header"),
        "wrong CRC": ([blocks[0] + bgzf_block(raw[200:], crc=zlib.crc32(raw[200:]) ^ 1)], ["a"], [300], -4, "CRC mismatch"),
        "wrong CRC in a gzip stream": ([gz[:-8] + struct.pack("<II", zlib.crc32(raw) ^ 1, len(raw))], ["a"], [300], -4, "Failed to decompress"),
        "wrong ISIZE": ([blocks[0] + bgzf_block(raw[200:], isize=len(raw) - 200 - 1)], ["a"], [300], -4, "ISIZE"),
        "ISIZE too large": ([blocks[0] + bgzf_block(raw[200:], isize=len(raw) - 200 + 1)], ["a"], [300], -4, "ISIZE"),
        "wrong ISIZE in a gzip stream": ([gz[:-4] + struct.pack("<I", len(raw) + 1)], ["a"], [300], -4, "Failed to decompress"),
        "BSIZE past the end": ([blocks[0] + bgzf_block(raw[200:], bsize=60000)], ["a"], [300], -4, "BSIZE leads outside the file"),
    }
    out = {}
    for key, (blobs, names, lens, code, words) in cases.items():
        paths = [put(tmp_path, "%s.%d" % (key.replace(" ", "_").replace("'", ""), k), b) for k, b in enumerate(blobs)]
        out[key] = (paths, names, lens, code, words)
    out["unreadable"] = ([str(tmp_path / "no_such_file.fa")], ["a"], [4], -4, "no_such_file.fa")
    return out
