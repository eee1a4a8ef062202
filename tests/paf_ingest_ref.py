"""A plain Python model of what the streamed PAF ingest hands to the index builder (impg_gpu_index_create_from_paf_streamed,
impg_gpu_selftest_paf_ingest): the reference's parse_paf_line / parse_paf (paf.rs:118-194) and its CIGAR tokens
(impg.rs:2935-2950) restated line by line, with the rules host_ingest.cpp's comments add: numbers are an optional '+' and
digits with 64-bit wrap, coordinates keep their low 32 bits, an op is (code << 29) | len unmasked, the first length seen
for a name wins, ids run in first-seen order over the files (query before target on a line).  Written from the reference
and those comments, not from the code under test.

One rule is the streamed route's own: the call fails with the message of the FIRST bad line in file order, a line's head
checks before its CIGAR check (the host route tokenises last and reports a bad head anywhere before any bad CIGAR)."""
OP_CHARS = b"=XIDM"
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


class ParseError(Exception):
    pass


def to_u64(f):
    """usize::from_str as the host parser has it: optional '+', then digits only, at least one; None: not a number"""
    d = f[1:] if f[:1] == b"+" else f
    if not d or any(c < 48 or c > 57 for c in d):
        return None
    v = 0
    for c in d:
        v = (v * 10 + (c - 48)) & M64
    return v


def i32(v):
    v &= M32
    return v - (1 << 32) if v >= (1 << 31) else v


def tokens(cigar):
    """every non-digit byte closes an op; digits behind the last letter are dropped; None: a byte that is no op letter"""
    out, n = [], 0
    for c in cigar:
        if 48 <= c <= 57:
            n = (n * 10 + (c - 48)) & M32
            continue
        code = OP_CHARS.find(bytes([c]))
        if code < 0:
            return None
        out.append(((code << 29) | n) & M32)
        n = 0
    return out


def lines_of(text):
    """BufRead::lines: split at '\\n', a '\\r' before it stripped, no line behind a final '\\n'"""
    if not text:
        return []
    body = text[:-1] if text.endswith(b"\n") else text
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in body.split(b"\n")]


def ingest(texts):
    """texts: the files' bytes -> dict(records, ops, names, lens, file_first); raises ParseError with the route's message.
    A record is (query_id, target_id, query_start, query_end, target_start, target_end, cigar_off, cigar_len, strand)."""
    names, lens, ids = [], [], {}
    records, ops, file_first = [], [], []

    def seq_id(name, length):
        if name not in ids:
            ids[name] = len(names)
            names.append(name)
            lens.append(length - (1 << 64) if length >= (1 << 63) else length)
        return ids[name]

    for text in texts:
        file_first.append(len(records))
        for line in lines_of(text):
            f = line.split(b"\t")
            if len(f) < 12:
                raise ParseError("Failed to parse PAF: Not enough fields in PAF record")
            nums = [to_u64(f[k]) for k in (1, 2, 3, 6, 7, 8)]
            if any(v is None for v in nums):
                raise ParseError("Failed to parse PAF: Invalid field")
            if not f[4]:
                raise ParseError("Failed to parse PAF: Expected '+' or '-' for strand")
            if f[4][:1] not in (b"+", b"-"):
                raise ParseError("Failed to parse PAF: Invalid strand")
            cigar = next((x[5:] for x in f if x.startswith(b"cg:Z:")), b"")
            t = tokens(cigar)
            if t is None:
                raise ParseError("Failed to parse PAF: Invalid CIGAR operation")
            q = seq_id(f[0], nums[0])
            tg = seq_id(f[5], nums[3])
            records.append((q, tg, i32(nums[1]), i32(nums[2]), i32(nums[4]), i32(nums[5]), len(ops), len(t), 1 if f[4][:1] == b"-" else 0))
            ops.extend(t)
    file_first.append(len(records))
    return dict(records=records, ops=ops, names=names, lens=lens, file_first=file_first)
