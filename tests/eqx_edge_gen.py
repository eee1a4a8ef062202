"""Fixtures that put the resolve pass's kernels (impg_amd/csrc/cigar_resolve_device.hip) on the edges of their own geometry:
the shipped tile of 1024 bases and the widest of 4096, chunk counts that the loop of four chunks does not divide, runs that
cross thousands of tiles through the back-to-front scan, '=' / 'X' ops longer than a tile, records without ops wherever the
searches over the records' first ops can meet them.  Built like tests/eqx_gen.py's and held to the same model
(tests/eqx_ref.py), but in numpy, and with every op's differ mask kept, so that geometry() can say where a fixture's starts,
tiles, chunks and chains lie.  The old fixtures and their caps stay as they are; this module's caps: a fixture has at most
MAX_RECORDS records and its sequences at most MAX_BASES bases each."""
import numpy as np

from tests import eqx_gen as gen, eqx_ref as ref

MAX_RECORDS = 700
MAX_BASES = 13000000

_UNLIKE = np.full(256, ord("A"), dtype=np.uint8)  # eqx_gen.differ_from as a table
for _a, _b in zip(b"ACGTacgt", b"CGTACGTA"):
    _UNLIKE[_a] = _b


class Fixture(gen.Fixture):
    """eqx_gen.Fixture whose record() works on arrays; masks[(record, op)] = the differ mask of every '=' 'X' 'M' op of a
    record written with its cg:Z, cases[record] = whatever the builder wants to say about it"""

    def __init__(self, seed):
        super().__init__(seed)
        self.masks, self.cases = {}, {}

    def record(self, qname, tname, ts, ops, strand="+", gap=0, cigar=True, claim=None, case=None):
        T = np.frombuffer(bytes(self.seqs[tname][ts:ts + sum(n for c, n, _ in ops if c != "I")]), dtype=np.uint8)
        parts, t = [], 0
        for k, (code, n, differ) in enumerate(ops):
            if code in "=XM":
                d = np.full(n, code == "X", dtype=bool) if differ is None else np.asarray(differ, dtype=bool)
                assert len(d) == n and t + n <= len(T)
                seg = T[t:t + n].copy()
                seg[d] = _UNLIKE[seg[d]]
                parts.append(seg)
                if cigar:
                    nd = int(d.sum())
                    if code == "M":
                        self.planted["m_x"] += nd
                        self.planted["m_eq"] += n - nd
                    elif code == "=":
                        self.planted["bad_eq"] += nd
                    else:
                        self.planted["bad_x"] += n - nd
                    self.masks[(len(self.rows), k)] = d
                t += n
            elif code == "I":
                parts.append(np.frombuffer(self.random(n), dtype=np.uint8))
            else:
                t += n
        seg = np.concatenate(parts).tobytes() if parts else b""
        Q = self.seqs.setdefault(qname, bytearray())
        Q += self.random(gap)
        qs = len(Q)
        Q += ref.comp(seg.upper())[::-1] if strand == "-" else seg
        dt, dq = claim or (0, 0)
        if case is not None:
            self.cases[len(self.rows)] = case
        self.rows.append((qname, qs, len(Q) + dq, strand, tname, ts, ts + t + dt, "".join("%d%s" % (n, c) for c, n, _ in ops) if cigar else None))


def at(n, *positions):
    return gen.at(n, *positions)


def geometry(records, ops, flags, differ_masks, tile, detail=True):
    """How the pass cuts its work at `tile` bases, and nothing else: no op is written here.
    differ_masks[(record, op in the record)]: a bool array, the positions of the op whose bases differ.
    -> dict(items   the items of all ops: max(1, ceil(len / tile)) for an '=', 'X' or 'M' of a resolvable record, else 1,
            tiles   (detail) a dict per tile of those ops: record, op, code, k, bases, chunks = ceil(bases / 64) and, for an 'M',
                    starts: the positions in the tile that start a run -- position 0 of the op, or a class unlike the
                    position before (None for '=' / 'X'),
            chains  the length of every maximal chain of an 'M' op's tiles without a start)"""
    items, tiles, chains = 0, [], []
    for i, r in enumerate(records):
        a = int(r["cigar_off"])
        for k in range(int(r["cigar_len"])):
            code, n = int(ops[a + k]) >> 29, int(ops[a + k]) & ref.LEN_MASK
            if flags[i] or code not in (0, 1, 4):
                items += 1
                continue
            nt = max(1, -(-n // tile))
            items += nt
            starts = per = None
            if code == 4 and n:
                d = np.asarray(differ_masks[(i, k)], dtype=bool)
                assert len(d) == n
                starts = np.concatenate(([0], np.flatnonzero(d[1:] != d[:-1]) + 1))
                per = np.bincount(starts // tile, minlength=nt)
                z = np.concatenate(([False], per == 0, [False]))
                edge = np.flatnonzero(z[1:] != z[:-1])
                chains.extend((edge[1::2] - edge[::2]).tolist())
            if detail and n:
                mine = np.split(starts, np.cumsum(per)[:-1]) if starts is not None else [None] * nt
                for t in range(nt):
                    bases = min(tile, n - t * tile)
                    tiles.append(dict(record=i, op=k, code=code, k=t, bases=bases, chunks=-(-bases // 64),
                                      starts=None if mine[t] is None else (mine[t] - t * tile).tolist()))
    return dict(items=items, tiles=tiles, chains=chains)


# ---- wide: the shipped tile and the wide ones ---------------------------------------------------------------------------------
WIDE_TILES = (1024, 2048, 4096)
WIDE_CHUNKS = (1, 3, 4, 5)  # ... and nch - 1: chunk borders on both sides of the loop's four chunks, and the tile's last


def wide_lengths(T):
    """the issue's six, 3T+1 (a last tile of one base), 2T+63 (of 63) and 2T+421 (of seven chunks, the last of 37 bases)"""
    return (T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 7, 3 * T + 1, 2 * T + 63, 2 * T + 421)


def wide_patterns(T, L):
    """[(name, differ mask)] of a single M of L bases meant for tiles of T"""
    pats = [("none", at(L)), ("all", np.ones(L, dtype=bool)), ("first", at(L, 0)), ("last", at(L, L - 1)), ("alternating", np.arange(L) % 2 == 0)]
    if L in (T + 1, 2 * T + 1, 3 * T + 7):
        pats += [("tile-", at(L, T - 1)), ("tile+", at(L, T)), ("tile-+", at(L, T - 1, T))]
    # chunk borders of one tile: tile 0 of L = T, tile 1 of L = 3T+7 (both of T / 64 full chunks), the last tile of L = 2T+421
    b, nch = {T: (0, T // 64), 3 * T + 7: (T, T // 64), 2 * T + 421: (2 * T, 7)}.get(L, (0, 0))
    for c in (WIDE_CHUNKS + (nch - 1,)) if nch else ():
        p = b + 64 * c
        pats += [("chunk%d-" % c, at(L, p - 1)), ("chunk%d+" % c, at(L, p)), ("chunk%d-+" % c, at(L, p - 1, p))]
    if L in (T, 3 * T + 7):
        pats.append(("next", at(L, b + 5, b + T - 3)))  # the start at b+6 ends at b+T-3: chunk 0's `nxt` comes from the tile's last chunk
    if L == 3 * T + 7:
        pats.append(("tail", np.arange(L) >= 2 * T + 10))  # starts at 0 and 2T+10 only: tiles 1 and 3 have none, tile 2 has one
    return pats


def wide():
    """single-M records of one to four tiles of 1024, 2048 and 4096 bases, the mismatches on, before and behind the borders
    of the tile, of its 64-base chunks and of the loop that loads four chunks at a time"""
    fx = Fixture(201)
    fx.sequence("T", 17 + 3 * 4096 + 7)
    i = 0
    for T in WIDE_TILES:
        for L in wide_lengths(T):
            for pat, d in wide_patterns(T, L):
                for strand in "+-":
                    fx.record("Q%d" % T, "T", gen.BORDER_STARTS[i % 5], [("M", L, d)], strand, case=(T, L, pat, strand))  # (no gap, as borders)
                    i += 1
    return fx


# ---- chains: runs across more tiles than rocPRIM scans in three blocks ------------------------------------------------------
# rocprim/device/detail/config/device_scan.hpp names no configuration for gfx950; the largest block that any of its
# specialisations for a 4-byte value names is gfx942's for float, line 921: scan_config<256, 24, ...> = 6144 values (gfx942's
# for int, line 976, has 256 x 21 = 5376; the unspecialised default 256 x 16 = 4096).
SCAN_BLOCK = 256 * 24
CHAIN_TILES = 3 * SCAN_BLOCK                # C: tiles of 64 bases without a start, one behind the other
CHAIN_BASES = 64 * (CHAIN_TILES + 32)       # an op's length: C + 32 tiles of 64, C / 16 + 2 tiles of 1024
CHAIN_LEAD = (0, 1, 2, 3)                   # one-base records in front of the long ones, in turn


def chains():
    """single-M records of 64 * (C + 32) bases, C = 3 * 6144 tiles (see SCAN_BLOCK): all equal, all different, one mismatch at
    the very last position, one in the middle (two chains), one run that ends at the last position of tile C + 15 of 64 (tile
    C / 16 of 1024); each on both strands, with 0, 1, 2, 3, 0, ... one-base records in front, so that the chains begin at every
    place of the blocks of four waves"""
    fx = Fixture(202)
    L = CHAIN_BASES
    fx.sequence("T", L + 64)
    pats = [("none", at(L)), ("all", np.ones(L, dtype=bool)), ("last", at(L, L - 1)), ("middle", at(L, L // 2 + 21)),
            ("tile end", np.arange(L) >= 64 * (CHAIN_TILES + 16))]
    i = 0
    for pat, d in pats:
        for strand in "+-":
            for _ in range(CHAIN_LEAD[i % 4]):
                fx.record("Q", "T", 7 * i, [("M", 1, at(1, 0) if i % 2 else None)], "+-"[i % 2])
            fx.record("Q", "T", gen.BORDER_STARTS[i % 5], [("M", L, d)], strand, case=(pat, strand))
            i += 1
    return fx


# ---- checked: '=' / 'X' ops longer than a tile, some of them lying ------------------------------------------------------------
CHECKED_TILES = (64, 1024)


def checked_lies(T, L):
    """[(name, positions)]: none; the op's first and last position; both sides of the tile border and of a chunk border
    that is no tile border at 1024; inside the last chunk where it is partial"""
    lies = [("none", ()), ("first", (0,)), ("last", (L - 1,)), ("tile-", (T - 1,)), ("tile+", (T,)), ("tile-+", (T - 1, T)),
            ("chunk-", (127,)), ("chunk+", (128,)), ("chunk-+", (127, 128))]
    if L % 64:
        lies.append(("partial", (L - L % 64 + (L % 64) // 2,)))
    return [(name, tuple(p for p in pos if 0 <= p < L)) for name, pos in lies]


def checked():
    """a PAF that is '=' / 'X' already: single-op records of about T and 2T+1 bases for T = 64 and 1024 whose op lies at known
    positions, an 'X' that is wholly a lie and an '=' that is wholly true across three tiles of 1024"""
    fx = Fixture(203)
    fx.sequence("C", 3200)
    i = 0
    for T in CHECKED_TILES:
        for L in (T - 1, T, T + 1, 2 * T + 1, 2 * T + 37):
            for name, pos in checked_lies(T, L):
                if len(pos) == 0 and name != "none":
                    continue
                for code in "=X":
                    for strand in "+-":
                        lie = at(L, *pos)
                        fx.record("QC%d" % T, "C", gen.BORDER_STARTS[i % 5] + 11 * (i % 7), [(code, L, lie if code == "=" else ~lie)], strand,
                                  case=(T, L, name, code, strand, len(pos)))
                        i += 1
    fx.record("QCw", "C", 3, [("X", 2 * 1024 + 9, at(2 * 1024 + 9))], "+", case=(1024, 2 * 1024 + 9, "all", "X", "+", 2 * 1024 + 9))
    fx.record("QCw", "C", 5, [("=", 3 * 1024, None)], "-", case=(1024, 3 * 1024, "none", "=", "-", 0))
    return fx


# ---- holes: records without ops, and a flagged one ----------------------------------------------------------------------------
HOLES_EMPTY = [1, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1]  # cigar_len == 0, record by record
HOLES_FLAGS = [0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0]


def holes():
    """records without cg:Z first, last, three in a row and between an M of 4096 bases and an M of one; an inconsistent record
    with one M of 5000 bases between two resolvable ones"""
    fx = Fixture(204)
    fx.sequence("T", 9000)
    rng = fx.rng
    m = lambda n, p: [("M", n, rng.random(n) < p)]
    fx.record("Q", "T", 10, m(200, 0.1), cigar=False)
    fx.record("Q", "T", 40, m(300, 0.05), "-", gap=2)
    for k in range(3):
        fx.record("Q", "T", 500 + 90 * k, m(80 + k, 0.2), "+-"[k % 2], gap=k, cigar=False)
    fx.record("Q", "T", 1, m(4096, 0.01), "+")
    fx.record("Q", "T", 4000, m(100, 0.3), "-", cigar=False)
    fx.record("Q", "T", 17, [("M", 1, at(1, 0))], "-")
    fx.record("Q", "T", 2000, m(200, 0.02) + [("I", 3, None)] + m(70, 0.5), "+", gap=1)
    fx.record("Q", "T", 3000, m(5000, 0.01), "-", claim=(1, 0))  # ops that do not add up: copied as one item
    fx.record("Q", "T", 6000, m(150, 0.1) + [("D", 4, None)] + m(1100, 0.01), "-")
    fx.record("Q", "T", 8000, m(500, 0.1), "+", cigar=False)
    return fx


FIXTURES = dict(wide=wide, chains=chains, checked=checked, holes=holes)
_CACHE = {}


def fixture(name):
    """as eqx_gen.fixture, with masks = the fixture's differ masks for geometry(); built once a process"""
    if name not in _CACHE:
        fx = FIXTURES[name]()
        paf, store = fx.paf(), fx.store()
        recs, ops, names, lens = ref.parse_paf(paf)
        assert len(recs) <= MAX_RECORDS and all(len(v) <= MAX_BASES for v in store.values())
        _CACHE[name] = dict(fx=fx, paf=paf, store=store, records=recs, ops=ops, names=names, seq_len=lens, masks=fx.masks,
                            model=ref.resolve(recs, ops, names, lens, store))
    return _CACHE[name]


def shuffled(f):
    """the records' ops reversed record by record in the pool: -> (records, pool); the pool out is the same"""
    rec = f["records"].copy()
    parts, at_ = [], 0
    for i in reversed(range(len(rec))):
        a, n = int(rec[i]["cigar_off"]), int(rec[i]["cigar_len"])
        parts.append(f["ops"][a:a + n])
        rec[i]["cigar_off"] = at_
        at_ += n
    return rec, np.concatenate(parts)


def shipped():
    """The end-to-end world at the shipped tile (TILE_BASES = 1024, which from_paf(resolve_matches=) always runs at): wide's
    records of 1024-base tiles and every fifth of checked's 1024-base ones with its two whole ops, as one PAF with its
    store, its model, the masks by its own record numbers, and 40 ranges (target id, start, end) that start inside records.
    Range 0 starts inside the second tile of wide's all-equal M of 3 * 1024 + 7 bases; range 1 ends inside the run of its M of
    2 * 1024 + 1 bases with one mismatch at 0, two bases behind the tile border that the run crosses."""
    if "shipped" not in _CACHE:
        w, c = fixture("wide"), fixture("checked")
        take = [(w, i) for i, case in sorted(w["fx"].cases.items()) if case[0] == 1024]
        of_c = [i for i, case in sorted(c["fx"].cases.items()) if case[0] == 1024]
        take += [(c, i) for k, i in enumerate(of_c[:-2]) if k % 5 == 0] + [(c, i) for i in of_c[-2:]]
        paf = "".join(f["paf"].splitlines()[i] + "\n" for f, i in take)
        store = {n: w["store"][n] for n in ("T", "Q1024")}
        store.update({n: c["store"][n] for n in ("C", "QC1024", "QCw")})
        recs, ops, names, lens = ref.parse_paf(paf)
        masks = {(k, 0): f["masks"][(i, 0)] for k, (f, i) in enumerate(take)}
        rng, ranges = np.random.default_rng(9), []
        find = lambda L, pat: next(k for k, (f, i) in enumerate(take) if f is w and f["fx"].cases[i] == (1024, L, pat, "+"))
        r = recs[find(3 * 1024 + 7, "none")]
        ranges.append((int(r["target_id"]), int(r["target_start"]) + 1024 + 100, int(r["target_start"]) + 1024 + 400))
        r = recs[find(2 * 1024 + 1, "first")]
        ranges.append((int(r["target_id"]), int(r["target_start"]) + 900, int(r["target_start"]) + 1024 + 3))
        for k in range(38):
            r = recs[(k * 7) % len(recs)]
            a = int(r["target_start"]) + int(rng.integers(0, max((int(r["target_end"]) - int(r["target_start"])) // 2, 1)))
            ranges.append((int(r["target_id"]), a, min(a + int(rng.integers(100, 500)), int(lens[r["target_id"]]))))
        _CACHE["shipped"] = dict(paf=paf, store=store, records=recs, ops=ops, names=names, seq_len=lens, masks=masks, ranges=ranges,
                                 model=ref.resolve(recs, ops, names, lens, store))
    return _CACHE["shipped"]


def fasta(store):
    return "".join(">%s\n%s\n" % (k, "\n".join(v[i:i + 70].decode() for i in range(0, len(v), 70))) for k, v in store.items())


ALL = tuple(FIXTURES)
