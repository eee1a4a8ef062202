"""The resolve pass (impg_gpu_cigar_resolve, include/impg_gpu.h) restated in plain Python: every
'M' op of a record rewritten as the '=' / 'X' runs its two sequences spell.  This file and the issue's text are the definition
the host twin and the kernels are held to.

A record with ops is resolvable iff both its sequences are in the store, their stored lengths equal seq_len, 0 <= start <=
end <= len on both axes, every op code is <= 4, the '=' 'X' 'M' 'D' lengths sum to target_end - target_start and the '=' 'X' 'M'
'I' lengths to query_end - query_start.  Otherwise: flag 1 if a sequence is absent from the store, else flag 2, ops copied.
Cursors t, q start at 0; '=' 'X' 'M' advance both, 'I' q, 'D' t.  Target byte T[target_start + t]; query byte Q[query_start + q]
on '+', comp(Q[query_end - 1 - q]) on '-' (A<->T, C<->G, every other byte itself; the store is upper case).  Bytes equal =
match.  'M' of L > 0 -> its maximal runs as '=' (0) / 'X' (1) ops; 'M' of 0 -> one '=' of 0; the other ops verbatim; nothing
fused across op borders.  New pool in record order, cigar_off = the ops of the records before."""
import numpy as np

CODES = "=XIDM"
LEN_MASK = (1 << 29) - 1
REPORT_FIELDS = ("records", "resolved", "absent", "inconsistent", "ops_in", "ops_out", "m_ops", "m_bases", "m_eq_bases", "m_x_bases",
                 "bad_eq_bases", "bad_x_bases")
RECORD_DTYPE = np.dtype([("query_id", "<u4"), ("target_id", "<u4"), ("query_start", "<i4"), ("query_end", "<i4"),
                         ("target_start", "<i4"), ("target_end", "<i4"), ("cigar_off", "<u8"), ("cigar_len", "<u4"),
                         ("strand", "<u4")], align=True)
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in (("A", "T"), ("C", "G")):
    _COMP[ord(_a)], _COMP[ord(_b)] = ord(_b), ord(_a)


def comp(seq):
    """the complement of upper-case bytes, position by position (no reversal)"""
    return _COMP[np.frombuffer(bytes(seq), dtype=np.uint8)].tobytes()


def pack(cigar):
    """'3=1X' -> packed ops"""
    out, n = [], ""
    for ch in cigar:
        if ch.isdigit():
            n += ch
        else:
            out.append(CODES.index(ch) << 29 | int(n))
            n = ""
    return np.array(out, dtype=np.uint32)


def unpack(ops):
    return "".join("%d%s" % (int(w) & LEN_MASK, CODES[int(w) >> 29]) for w in ops)


def runs(differ):
    """a bool array -> [(class, length)] of its maximal runs"""
    if len(differ) == 0:
        return []
    cut = np.flatnonzero(differ[1:] != differ[:-1]) + 1
    edges = np.concatenate(([0], cut, [len(differ)]))
    return [(int(differ[a]), int(b - a)) for a, b in zip(edges[:-1], edges[1:])]


def flag_of(r, ops, names, seq_len, store):
    if r["cigar_len"] == 0:
        return 0
    q, t = store.get(names[r["query_id"]]), store.get(names[r["target_id"]])
    if q is None or t is None:
        return 1
    if len(q) != seq_len[r["query_id"]] or len(t) != seq_len[r["target_id"]]:
        return 2
    if not (0 <= r["query_start"] <= r["query_end"] <= len(q) and 0 <= r["target_start"] <= r["target_end"] <= len(t)):
        return 2
    st = sq = 0
    for w in ops:
        code, n = int(w) >> 29, int(w) & LEN_MASK
        if code > 4:
            return 2
        st += n if code != 2 else 0
        sq += n if code != 3 else 0
    if st != r["target_end"] - r["target_start"] or sq != r["query_end"] - r["query_start"]:
        return 2
    return 0


def resolve(records, ops, names, seq_len, store):
    """store: {name: bytes as the FASTA holds them}.  -> (records, ops, flags, report) as impg_gpu_cigar_resolve returns them"""
    store = {k: bytes(v).upper() for k, v in store.items()}
    rep = dict.fromkeys(REPORT_FIELDS, 0)
    rep["records"] = len(records)
    out_rec = np.array(records, dtype=RECORD_DTYPE)
    out, flags = [], np.zeros(len(records), dtype=np.uint8)
    for i, r in enumerate(records):
        mine = np.asarray(ops[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])], dtype=np.uint32)
        first = len(out)
        rep["ops_in"] += len(mine)
        flags[i] = f = flag_of(r, mine, names, seq_len, store)
        if len(mine):
            rep[("resolved", "absent", "inconsistent")[f]] += 1
        if f or not len(mine):
            out.extend(int(w) for w in mine)
        else:
            T = np.frombuffer(store[names[r["target_id"]]], dtype=np.uint8)[int(r["target_start"]):int(r["target_end"])]
            Q = np.frombuffer(store[names[r["query_id"]]], dtype=np.uint8)[int(r["query_start"]):int(r["query_end"])]
            if r["strand"]:
                Q = _COMP[Q[::-1]]
            t = q = 0
            for w in mine:
                code, n = int(w) >> 29, int(w) & LEN_MASK
                if code in (0, 1, 4):
                    differ = T[t:t + n] != Q[q:q + n]
                    assert len(differ) == n
                    nx = int(differ.sum())
                if code == 4:
                    rep["m_ops"] += 1
                    rep["m_bases"] += n
                    rep["m_x_bases"] += nx
                    rep["m_eq_bases"] += n - nx
                    out.extend((c << 29 | ln) for c, ln in runs(differ)) if n else out.append(0)
                else:
                    out.append(int(w))
                    if code == 0:
                        rep["bad_eq_bases"] += nx
                    if code == 1:
                        rep["bad_x_bases"] += n - nx
                t += n if code != 2 else 0
                q += n if code != 3 else 0
        out_rec[i]["cigar_off"], out_rec[i]["cigar_len"] = first, len(out) - first
    rep["ops_out"] = len(out)
    return out_rec, np.array(out, dtype=np.uint32), flags, rep


def fuse_back(ops_in, ops_out):
    """the model's output with its '=' / 'X' runs fused wherever the input had an 'M': the input again, or None"""
    back, k = [], 0
    for w in ops_in:
        code, n = int(w) >> 29, int(w) & LEN_MASK
        if code != 4:
            if k >= len(ops_out) or int(ops_out[k]) != int(w):
                return None
            back.append(int(w))
            k += 1
            continue
        got = 0
        while True:
            if k >= len(ops_out) or int(ops_out[k]) >> 29 > 1:
                return None
            got += int(ops_out[k]) & LEN_MASK
            k += 1
            if got >= n:
                break
        if got != n:
            return None
        back.append(4 << 29 | n)
    return back if k == len(ops_out) else None


# ---- PAF text ------------------------------------------------------------------------------------------------------------
def parse_paf(text):
    """-> (records, ops, names, seq_len): ids in first-seen order, query then target, a line after the other"""
    names, lens, ids = [], [], {}

    def sid(name, n):
        if name not in ids:
            ids[name] = len(names)
            names.append(name)
            lens.append(n)
        return ids[name]

    recs, pool = [], []
    for line in text.splitlines():
        f = line.split("\t")
        q = sid(f[0], int(f[1]))
        t = sid(f[5], int(f[6]))
        cg = [x[5:] for x in f[12:] if x.startswith("cg:Z:")]
        mine = pack(cg[0]) if cg else np.zeros(0, dtype=np.uint32)
        recs.append((q, t, int(f[2]), int(f[3]), int(f[7]), int(f[8]), len(pool), len(mine), 1 if f[4] == "-" else 0))
        pool.extend(int(w) for w in mine)
    return np.array(recs, dtype=RECORD_DTYPE), np.array(pool, dtype=np.uint32), names, np.array(lens, dtype=np.int64)


def convert_paf(text, store):
    """the same lines with every cg:Z: rewritten by the model; flagged records are left as they are"""
    recs, pool, names, lens = parse_paf(text)
    out_rec, out, flags, rep = resolve(recs, pool, names, lens, store)
    lines = []
    for i, line in enumerate(text.splitlines()):
        f = line.split("\t")
        for k in range(12, len(f)):
            if f[k].startswith("cg:Z:") and not flags[i]:
                a = int(out_rec[i]["cigar_off"])
                f[k] = "cg:Z:" + unpack(out[a:a + int(out_rec[i]["cigar_len"])])
        lines.append("\t".join(f))
    return "".join(ln + "\n" for ln in lines)
