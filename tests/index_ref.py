"""An independent model of the built index: what GpuImpg.save writes, parsed back into named arrays (read_index), the
same arrays built the slow, obvious way from records and packed ops (expected_index), and a comparison that names the
first differing blob, element and field (diff_index).

Plain Python / numpy; nothing here imports the library.  The arrays follow the layout comments of
impg_amd/csrc/impg_internal.hpp (op line, prefix line, identity line, Entry, SegDesc) and the reference's ordering rule
(Impg::from_multi_alignment_records pushes a record's forward entry, then its reversed one, and BasicCOITree::new sorts
each target's intervals stably by their signed 32-bit start, impg.rs:1559-1630), not either builder's code.  All running
sums are unsigned 32-bit, as the layout's words are.

Not modelled: blobs 7 and 8 (rank, mrank).  Both builders take them from one host function; tests/test_oracle_kat.py and
the parity tests own their values.  check_ranks() only asks that they are a permutation of 0..n-1 in every segment.

Conventions the layout comments leave open and this model fixes: a segment's sampled levels are stored one after the
other in sequence-id order (level 1 of target 0, level 2 of target 0, level 1 of target 1 ...), and the external
checkpoints of the entries follow each other in entry order."""
import struct

import numpy as np

M32 = 0xFFFFFFFF
TILE_WORDS, TILE_OPS, TILE_SUBS, INLINE_TILES, MAX_LEVELS = 32, 26, 4, 8, 4
SUB_FIRST_OP = (0, 6, 14, 22)
OP_PAD = 0xE0000000
OP_LEN_MASK = (1 << 29) - 1
EF_STRAND, EF_REVERSED = 1 << 30, 1 << 31
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
MAGIC = b"IMPGHBM1"
VERSION = 6
END_MARK = 0x454E44474D50
FNV_SEED, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3

SEG_DTYPE = np.dtype([("a", "<u4"), ("n", "<u4"), ("nlev", "<u4"), ("off", "<u4", (MAX_LEVELS,)), ("cnt", "<u4", (MAX_LEVELS,)), ("pad", "<u4")])
ENTRY_DTYPE = np.dtype([("ts", "<i4"), ("te", "<i4"), ("qs", "<i4"), ("qe", "<i4"), ("query_id", "<u4"), ("tile_base", "<u4"),
                        ("nops_flags", "<u4"), ("totT", "<u4"), ("totQ", "<u4"), ("tcp", "<u4", (7,))])
assert SEG_DTYPE.itemsize == 48 and ENTRY_DTYPE.itemsize == 64
RECORD_DTYPE = np.dtype([("query_id", "<u4"), ("target_id", "<u4"), ("query_start", "<i4"), ("query_end", "<i4"),
                         ("target_start", "<i4"), ("target_end", "<i4"), ("cigar_off", "<u8"), ("cigar_len", "<u4"),
                         ("strand", "<u4")], align=True)
BLOB_NAMES = ("seg", "starts", "ends", "ends_t", "pmax", "starts_lvl", "pmax_lvl", "rank", "mrank", "entries", "op_lines",
              "ext_cp", "idl", "seq_len", "pfx")
MODELLED = tuple(n for n in BLOB_NAMES if n not in ("rank", "mrank"))
HEADER = struct.Struct("<8s8I7Q15Q")
HEADER_FIELDS = ("version", "tile_words", "tile_ops", "tile_subs", "entry_bytes", "n_seq", "sorted_order", "flags",
                 "n_records", "n_entries", "n_tiles", "n_targets", "n_names", "n_file_first", "n_tgt_off")
# header word `multi_file`, by bit
F_MULTI_FILE, F_TP, F_NO_PFX, F_SHARD, F_FRONT, F_LAZY_IDL = 1, 2, 4, 8, 16, 32
assert HEADER.size == 216


def fnv64(h, data):
    """FNV-1a over the 8-byte little-endian words of one write, then over its tail bytes."""
    b = bytes(data)
    n8 = len(b) // 8
    for w in np.frombuffer(b, dtype="<u8", count=n8).tolist():
        h = ((h ^ w) * FNV_PRIME) & 0xFFFFFFFFFFFFFFFF
    for c in b[8 * n8:]:
        h = ((h ^ c) * FNV_PRIME) & 0xFFFFFFFFFFFFFFFF
    return h


def _shape_blob(k, raw, flags):
    if k == 0:
        return np.frombuffer(raw, dtype=SEG_DTYPE)
    if k in (1, 2, 3, 4, 5, 6, 13):
        return np.frombuffer(raw, dtype="<i4")
    if k == 9:
        return np.frombuffer(raw, dtype=ENTRY_DTYPE)
    if k in (10, 14):
        return np.frombuffer(raw, dtype="<u4").reshape(-1, TILE_WORDS)
    if k == 12:
        return np.frombuffer(raw, dtype="<u4").reshape(-1, 4 if flags & F_NO_PFX else TILE_WORDS)
    return np.frombuffer(raw, dtype="<u4")


def read_index(path, check_sum=True):
    """The saved index as a dict: the header's fields, `lens`, `names`, `file_first`, `tgt_off`, `shard` (None or
    dict(world, rank, owner)) and one array per blob under BLOB_NAMES.  The end mark is always checked; the FNV sum
    (one pass of interpreted Python over every 8-byte word) unless check_sum is False."""
    data = open(path, "rb").read()
    pos = [0]
    h = [FNV_SEED]

    def take(n):
        if pos[0] + n > len(data):
            raise ValueError("%s is truncated" % path)
        b = data[pos[0]:pos[0] + n]
        pos[0] += n
        if check_sum:
            h[0] = fnv64(h[0], b)
        return b

    hd = HEADER.unpack(take(HEADER.size))
    if hd[0] != MAGIC:
        raise ValueError("bad magic")
    out = dict(zip(HEADER_FIELDS, hd[1:16]))
    blob_bytes = hd[16:]
    if (out["version"], out["tile_words"], out["tile_ops"], out["tile_subs"], out["entry_bytes"]) != (VERSION, TILE_WORDS, TILE_OPS, TILE_SUBS, 64):
        raise ValueError("another index layout")
    out["lens"] = np.frombuffer(take(8 * out["n_seq"]), dtype="<i8")
    names = []
    for _ in range(out["n_names"]):
        (n,) = struct.unpack("<I", take(4))
        names.append(take(n).decode())
    out["names"] = names
    out["file_first"] = np.frombuffer(take(8 * out["n_file_first"]), dtype="<u8")
    out["tgt_off"] = np.frombuffer(take(4 * out["n_tgt_off"]), dtype="<u4")
    out["shard"] = None
    if out["flags"] & F_SHARD:
        world, rank, n_owner = struct.unpack("<3I", take(12))
        out["shard"] = dict(world=world, rank=rank, owner=np.frombuffer(take(4 * n_owner), dtype="<u4"))
    for k, name in enumerate(BLOB_NAMES):
        out[name] = _shape_blob(k, take(blob_bytes[k]), out["flags"])
    out["blob_bytes"] = tuple(blob_bytes)
    (tail,) = struct.unpack("<Q", take(8))
    if tail != END_MARK ^ out["n_entries"]:
        raise ValueError("bad end mark")
    want_sum = h[0]  # (the sum covers the end mark too)
    (got_sum,) = struct.unpack("<Q", data[pos[0]:pos[0] + 8])
    if check_sum and got_sum != want_sum:
        raise ValueError("bad checksum")
    if pos[0] + 8 != len(data):
        raise ValueError("bytes behind the checksum")
    return out


def _tile_lines(opv, prefix_lines, identity_lines, carry):
    """One tile's op line, prefix line and identity words from its ops (Python ints) and the record's sums before it,
    carry = [T, Q, M, X, G].  Returns (op_line, pfx_line | None, idl | None, sub_rows | None) and advances carry."""
    t0, q0, m0, x0, g0 = carry
    cnt = len(opv)
    T, Q, Mm, X, G = carry
    before = []  # sums before op u
    gapmask = 0
    for u, v in enumerate(opv):
        before.append((T, Q, Mm, X, G))
        code, ln = v >> 29, v & OP_LEN_MASK
        if code > 4:
            raise ValueError("Invalid CIGAR operation")
        if code != 2:
            T = (T + ln) & M32
        if code != 3:
            Q = (Q + ln) & M32
        if code in (0, 4):
            Mm = (Mm + ln) & M32
        elif code == 1:
            X = (X + ln) & M32
        else:
            G = (G + 1) & M32
            gapmask |= 1 << u
    end = (T, Q, Mm, X, G)
    carry[:] = end
    at = lambda u: before[u] if u < cnt else end  # noqa: E731
    line = [t0, q0, 0, 0, 0, 0] + list(opv) + [OP_PAD] * (TILE_OPS - cnt)
    dT = [(at(f)[0] - t0) & M32 for f in (6, 14, 22)] + [(T - t0) & M32]
    dQ = [(at(f)[1] - q0) & M32 for f in (6, 14, 22)] + [(Q - q0) & M32]
    if dT[3] >= 0xFFFF or dQ[3] >= 0xFFFF:
        line[2:6] = [M32] * 4
    else:
        line[2:6] = [(dT[0] | dT[1] << 16) & M32, (dT[2] | dT[3] << 16) & M32, (dQ[0] | dQ[1] << 16) & M32, (dQ[2] | dQ[3] << 16) & M32]
    pfx = idl = subs = None
    if prefix_lines:
        rel = [((at(k)[0] - t0) & M32, (at(k)[1] - q0) & M32) for k in range(28)]
        wide = any(a > 0xFFFF or b > 0xFFFF for a, b in rel[:cnt]) or dT[3] > 0xFFFF or dQ[3] > 0xFFFF
        ent = [((a & 0xFFFF) | (b << 16)) & M32 for a, b in rel]
        pfx = [t0 | (1 << 31 if wide else 0), q0, ent[9], ent[18]] + ent
        if identity_lines:
            ient = [(((at(k)[2] - m0) & 0xFFFF) | (((at(k)[3] - x0) & M32) << 16)) & M32 for k in range(28)]
            idl = [m0, x0, g0, gapmask] + ient
    else:
        subs = [[at(f)[2], at(f)[3], at(f)[4], 0] for f in SUB_FIRST_OP]
    return line, pfx, idl, subs


def expected_index(records, ops, seq_len, bidirectional, prefix_lines=True, identity_lines=False, owner=None, shard=0, lines=True):
    """The blobs of MODELLED for these inputs.  lines=False: only seg, the columns, the levels and seq_len (the
    262 145-entry fixture, whose lines are compared host against device)."""
    rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    seq_len = np.asarray(seq_len, dtype=np.int64)
    n_seq, n_rec = len(seq_len), len(rec)
    own = np.ones(n_seq, dtype=bool) if owner is None else (np.asarray(owner) == shard)
    q, t = rec["query_id"].astype(np.int64), rec["target_id"].astype(np.int64)
    fwd = own[t] if n_rec else np.zeros(0, dtype=bool)
    rev = (own[q] & (q != t)) if (n_rec and bidirectional) else np.zeros(n_rec, dtype=bool)
    need = fwd | rev
    # entries in record order, the forward entry before the reversed one
    cnt = fwd.astype(np.int64) + rev.astype(np.int64)
    first = np.cumsum(cnt) - cnt
    e_rec = np.repeat(np.arange(n_rec), cnt)
    second = (np.arange(len(e_rec)) - first[e_rec]) == 1
    e_rev = second | ~fwd[e_rec]
    key_t = np.where(e_rev, q[e_rec], t[e_rec])
    key_s = np.where(e_rev, rec["query_start"][e_rec], rec["target_start"][e_rec]).astype(np.int32)
    order = np.lexsort((key_s, key_t))  # stable: ties keep record order
    e_rec, e_rev, key_t = e_rec[order], e_rev[order], key_t[order]
    n_ent = len(e_rec)
    ts = np.where(e_rev, rec["query_start"][e_rec], rec["target_start"][e_rec]).astype(np.int32)
    te = np.where(e_rev, rec["query_end"][e_rec], rec["target_end"][e_rec]).astype(np.int32)
    out = {"starts": ts, "ends": te, "ends_t": np.where(ts < te, te, np.int32(INT32_MIN)).astype(np.int32)}
    seg = np.zeros(n_seq, dtype=SEG_DTYPE)
    per = np.bincount(key_t, minlength=n_seq)[:n_seq] if n_ent else np.zeros(n_seq, dtype=np.int64)
    a = np.cumsum(per) - per
    pmax = np.zeros(n_ent, dtype=np.int32)
    lv_s, lv_p = [], []
    lvl_total = 0
    for s in range(n_seq):
        n = int(per[s])
        seg[s]["a"], seg[s]["n"] = a[s], n
        if n:
            pmax[a[s]:a[s] + n] = np.maximum.accumulate(te[a[s]:a[s] + n])
        cur_s, cur_p, lev = ts[a[s]:a[s] + n], pmax[a[s]:a[s] + n], 0
        while len(cur_s) > 64:
            last = np.minimum(64 * (np.arange((len(cur_s) + 63) // 64) + 1), len(cur_s)) - 1
            cur_s, cur_p = cur_s[last], cur_p[last]
            seg[s]["off"][lev], seg[s]["cnt"][lev] = lvl_total, len(cur_s)
            lv_s.append(cur_s)
            lv_p.append(cur_p)
            lvl_total += len(cur_s)
            lev += 1
        seg[s]["nlev"] = lev
    out["seg"], out["pmax"] = seg, pmax
    out["starts_lvl"] = np.concatenate(lv_s).astype(np.int32) if lv_s else np.zeros(0, dtype=np.int32)
    out["pmax_lvl"] = np.concatenate(lv_p).astype(np.int32) if lv_p else np.zeros(0, dtype=np.int32)
    out["seq_len"] = np.clip(seq_len, 0, INT32_MAX).astype(np.int32)
    out["tgt_off"] = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    if not lines:
        return out
    # tiles of every needed record, numbered over the needed records only
    tile_base = np.zeros(n_rec, dtype=np.int64)
    tot = np.zeros((n_rec, 2), dtype=np.int64)
    t0s, q0s = {}, {}  # record -> T0 / Q0 of its tiles
    op_lines, pfx_lines, idl_lines, sub_rows = [], [], [], []
    for i in np.nonzero(need)[0]:
        tile_base[i] = len(op_lines)
        off, n = int(rec["cigar_off"][i]), int(rec["cigar_len"][i])
        if off + n > len(ops):
            raise ValueError("record CIGAR outside the op pool")
        opv = ops[off:off + n].tolist()
        carry = [0, 0, 0, 0, 0]
        t0s[i], q0s[i] = [], []
        for k0 in range(0, n, TILE_OPS):
            t0s[i].append(carry[0])
            q0s[i].append(carry[1])
            line, pfx, idl, subs = _tile_lines(opv[k0:k0 + TILE_OPS], prefix_lines, identity_lines, carry)
            op_lines.append(line)
            if pfx is not None:
                pfx_lines.append(pfx)
            if idl is not None:
                idl_lines.append(idl)
            if subs is not None:
                sub_rows.extend(subs)
        tot[i] = carry[0], carry[1]
    n_tiles = len(op_lines)
    out["op_lines"] = np.array(op_lines, dtype=np.uint32).reshape(n_tiles, TILE_WORDS)
    out["pfx"] = np.array(pfx_lines, dtype=np.uint32).reshape(-1, TILE_WORDS)
    out["idl"] = (np.array(sub_rows, dtype=np.uint32).reshape(-1, 4) if not prefix_lines
                  else np.array(idl_lines, dtype=np.uint32).reshape(-1, TILE_WORDS))
    ent = np.zeros(n_ent, dtype=ENTRY_DTYPE)
    ext_cp = []
    for e in range(n_ent):
        i, rv = int(e_rec[e]), bool(e_rev[e])
        r = rec[i]
        n = int(r["cigar_len"])
        m = (n + TILE_OPS - 1) // TILE_OPS
        E = ent[e]
        if not rv:
            E["ts"], E["te"], E["qs"], E["qe"], E["query_id"] = r["target_start"], r["target_end"], r["query_start"], r["query_end"], r["query_id"]
            totT, totQ, starts = int(tot[i][0]), int(tot[i][1]), t0s[i]
        else:
            E["ts"], E["te"], E["qs"], E["qe"], E["query_id"] = r["query_start"], r["query_end"], r["target_start"], r["target_end"], r["target_id"]
            totT, totQ, starts = int(tot[i][1]), int(tot[i][0]), q0s[i]
        E["tile_base"] = tile_base[i]
        E["nops_flags"] = n | (EF_STRAND if r["strand"] else 0) | (EF_REVERSED if rv else 0)
        E["totT"], E["totQ"] = totT, totQ
        flip = rv and bool(r["strand"])

        def prefix(k):  # the entry's own target axis at the start of the k-th tile in the order the entry walks them
            if k == 0:
                return 0
            if k >= m:
                return totT
            # walked back to front, tile k starts where original tile m - k starts, measured from the record's end
            return (totT - starts[m - k]) & M32 if flip else starts[k]

        if m <= INLINE_TILES:
            E["tcp"] = [prefix(k) if k < m else totT if k == m else 0x7FFFFFFF for k in range(1, 8)]
        else:
            E["tcp"] = [len(ext_cp), 0, 0, 0, 0, 0, 0]
            ext_cp.extend(prefix(k) for k in range(m + 1))
    out["entries"] = ent
    out["ext_cp"] = np.array(ext_cp, dtype=np.uint32)
    return out


_LINE_WORDS = {"op_lines": lambda w: ("T0", "Q0", "dT1|dT2", "dT3|dT4", "dQ1|dQ2", "dQ3|dQ4")[w] if w < 6 else "op %d" % (w - 6),
               "pfx": lambda w: ("T0|wide", "Q0", "copy of entry 9", "copy of entry 18")[w] if w < 4 else "entry %d" % (w - 4)}


def _word_name(blob, w, width):
    if blob in _LINE_WORDS:
        return "word %d (%s)" % (w, _LINE_WORDS[blob](w))
    if blob == "idl" and width == TILE_WORDS:
        return "word %d (%s)" % (w, ("matched before", "mismatched before", "gap ops before", "gap mask")[w] if w < 4 else "entry %d" % (w - 4))
    if blob == "idl":
        return "word %d (%s)" % (w, ("matched", "mismatched", "gap ops", "zero")[w])
    return "word %d" % w


def diff_index(got, want, blobs=None):
    """None when every blob of `blobs` (default: those `want` holds, of MODELLED) is equal, else one line naming the first
    differing blob, its element (tile, entry, segment) and field (the word of a line, the member of Entry / SegDesc)."""
    for name in (blobs or [b for b in MODELLED if b in want]):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if g.shape != w.shape:
            return "%s: shape %s, expected %s" % (name, g.shape, w.shape)
        if g.dtype.names:
            for i in range(len(g)):
                if g[i] != w[i]:
                    for f in g.dtype.names:
                        if np.any(g[i][f] != w[i][f]):
                            return "%s[%d].%s: got %s, expected %s" % (name, i, f, g[i][f], w[i][f])
            continue
        bad = np.argwhere(g != w)
        if len(bad):
            idx = tuple(int(x) for x in bad[0])
            where = "%s[%d]" % (name, idx[0]) + (" " + _word_name(name, idx[1], g.shape[1]) if len(idx) > 1 else "")
            return "%s: got 0x%x, expected 0x%x" % (where, int(g[idx]) & M32, int(w[idx]) & M32)
    return None


def check_ranks(ix):
    """blobs 7 / 8: a permutation of 0..n-1 in every segment (mrank only where the index has several files)."""
    for name in ("rank", "mrank"):
        arr = ix[name]
        if name == "mrank" and len(arr) == 0:
            continue
        assert len(arr) == ix["n_entries"], name
        for s in ix["seg"]:
            a, n = int(s["a"]), int(s["n"])
            assert sorted(arr[a:a + n].tolist()) == list(range(n)), (name, a, n)
