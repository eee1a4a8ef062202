"""Inputs that put one (query, sequence) group of the visited update on a chosen tier, capacity edge or rare path, and a
plain model that says what each input reaches.

The model restates the proximity test (impg.rs:2513-2545), SortedRanges::insert with min_distance = 0 (impg.rs:270-368)
and the next-depth merge (impg.rs:2568-2584), and on top of them the engine's own bookkeeping: which kernel
big_groups_kernel hands the group to, where a wave's list leaves its LDS buffer, whether the pieces outnumber it, whether a
lane's pieces meet its list in the LDS column.  It is used only to say what an input reaches -- never as the expected
output of a query: that is the oracle's.

Every PAF here has three sequences.  One range on T covers H records whose query sides are H intervals on Q: level 1
replays exactly those H hits, in the records' order on T (the sorted visit order: build the index with ORDER_SORTED and
switch the oracle to its sorted policy), against the list the mask gives Q from the first touch (M ranges): cap = M + H,
old = M.  A few records Q -> R and R -> Q, the second shifted by six bases against the first, bring levels 3 and 4 back to
the same group with hits that partly overlap what is there."""
import bisect

# The engine's capacities, restated from kernels.hip.  The tiers and buffers (IMPG_VU_TINY_MAX, IMPG_VU_LDS_CAP, IMPG_VU_MID_MAX,
# IMPG_VU_MID_CAP, IMPG_VW_TINY, IMPG_VW_SMALL, VW_CAP_LARGE, VW_SMALL_HEADROOM; big_groups_kernel) are checked again by the
# update_* counters of tests/test_gpu_update_tiers.py.  The two grid sizes are NOT: they restate launch_visited_update's
# `mid_blocks = min(cdiv(n_groups, 64), 256 * min(32, 160 KB / (VU_MID_CAP * 64 * 8)))` blocks of 64 lanes and the tiny wave
# kernel's `min(n_groups, 256 * 32)` blocks -- whoever changes those two expressions changes MID_GRID / TINY_GRID here, or the
# many-mid / many-tiny cases stop reaching a second trip of the stride without any test noticing.
LANE_MAX, LANE_COL = 12, 12      # dense lane kernel: cap <= 12, a 12-entry LDS column
MID_MAX, MID_COL = 48, 64        # listed lane kernel: cap <= 48, a 64-entry column
WAVE_CAP = dict(tiny=192, small=1152, large=4096)  # the wave kernel's LDS buffer, in ranges / pieces
SMALL_OLD_MAX = 832              # old + 256 <= 1152 - 64
BATCH = 64                       # hits a wave takes per step; the list must have room for as many
MID_GRID = 256 * 5 * 64          # listed lane kernel: at most 1 280 blocks of 64 lanes, striding over the list
TINY_GRID = 256 * 32             # tiny wave kernel: at most 8 192 blocks, dealt round-robin
MTL = 2                          # min_transitive_len of every case that does not set its own


# ---- the plain model -----------------------------------------------------------------------------------------------------
def _lb(R, s):
    return bisect.bisect_left([r[0] for r in R], s)


def proximity_ok(R, s, e, mdbr):
    """impg.rs:2513-2545 (BFS: the next range is looked at only if the previous one did not reject)."""
    if mdbr <= 0:
        return True
    i = _lb(R, s)
    if i > 0 and abs(s - R[i - 1][1]) < mdbr:
        return False
    return not (i < len(R) and abs(R[i][0] - e) < mdbr)


def insert(R, s, e, seq_len):
    """SortedRanges::insert, min_distance = 0 (impg.rs:270-353) + merge_forward_from (:355-368).  Returns the
    not-yet-visited pieces and whether the list got one range longer."""
    s, e = max(min(s, e), 0), min(max(s, e), seq_len)            # :287-296
    out, cur = [], s
    i = _lb(R, s)                                                  # :303
    if i > 0 and R[i - 1][1] > s:
        i -= 1
    while i < len(R) and cur < e:                                  # :314-324
        if R[i][0] > e:
            break
        if cur < R[i][0]:
            out.append((cur, R[i][0]))
        cur = max(cur, R[i][1])
        i += 1
    if cur < e:
        out.append((cur, e))
    pos = _lb(R, s)                                                # :330-343
    if pos > 0 and R[pos - 1][1] >= s:
        R[pos - 1][1] = max(R[pos - 1][1], e)
        w = pos - 1
    elif pos < len(R) and e >= R[pos][0]:
        R[pos] = [min(s, R[pos][0]), max(e, R[pos][1])]
        w = pos
    else:
        R.insert(pos, [s, e])
        return out, True
    r = w + 1                                                      # :355-368
    while r < len(R) and R[w][1] >= R[r][0]:
        R[w][1] = max(R[w][1], R[r][1])
        r += 1
    del R[w + 1:r]
    return out, False


def merge_pieces(P):
    """impg.rs:2568-2584 for one (query, sequence): sort by start, merge overlapping / contiguous."""
    out = []
    for s, e in sorted(P, key=lambda p: p[0]):
        if out and out[-1][1] >= s:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def covered(R, s, e, seq_len):
    """covered_flags_kernel: one range of the list as the level found it covers the (clamped) hit."""
    s, e = max(s, 0), min(e, seq_len)
    i = _lb(R, s)
    return s < e and ((i < len(R) and R[i][0] == s and R[i][1] >= e) or (i > 0 and R[i - 1][1] >= e))


def tier_of(cap, old):
    """big_groups_kernel."""
    if cap <= LANE_MAX:
        return "lane"
    if cap <= MID_MAX:
        return "mid"
    if cap + BATCH <= WAVE_CAP["tiny"]:
        return "tiny"
    return "small" if old <= SMALL_OLD_MAX else "large"


def model(mask, hits, seq_len, mtl=MTL, mdbr=0, filter_covered=False):
    """What level 1 of the group reaches: dict(cap, old, tier, final_len, raw_pieces, pieces, leave, inplace, tiled, spill).
    leave = the hit index at which a wave's list leaves its LDS buffer (0: it never entered; None: it stays)."""
    R = [list(r) for r in mask]
    old = len(R)
    if filter_covered:
        hits = [h for h in hits if not covered(R, h[0], h[1], seq_len)]
    cap = old + len(hits)
    tier = tier_of(cap, old)
    col = LANE_COL if tier == "lane" else MID_COL
    P, spill, leave = [], False, None
    buf = WAVE_CAP.get(tier)
    if buf is not None and hits and old + BATCH > buf:
        leave = 0
    for t, (s, e) in enumerate(hits):
        if buf is not None and leave is None and t % BATCH == 0 and len(R) + BATCH > buf:
            leave = t
        if not proximity_ok(R, s, e, mdbr):
            continue
        before = len(R)
        new, grew = insert(R, s, e, seq_len)
        for a, b in new:
            if b - a >= mtl:
                if before + len(P) >= col:  # (the lane kernels: the piece's place in the column is the list's)
                    spill = True
                P.append((a, b))
        if grew and before + len(P) >= col:
            spill = True
    wave = buf is not None
    return dict(cap=cap, old=old, tier=tier, final_len=len(R), raw_pieces=len(P), pieces=len(merge_pieces(P)),
                leave=leave if wave else None, inplace=wave and leave is not None, tiled=wave and len(P) > buf,
                spill=(not wave) and spill)


# ---- cases ---------------------------------------------------------------------------------------------------------------
SP, X0, RL = 100, 200, 10  # slot spacing, first slot, length of a slot's range


def slot(i):
    return (X0 + i * SP, X0 + i * SP + RL)


def gap_hit(i):
    """An isolated hit in the gap behind slot i: 30 from the slot's range, 48 from the next."""
    return (X0 + i * SP + 40, X0 + i * SP + 52)


def shuffled(xs, mult=7919):
    n = len(xs)
    return [xs[(k * mult + 3) % n] for k in range(n)] if n > 1 and n % mult else list(xs)


def fillers(M, H, first=0):
    """H pairwise disjoint, non-touching hits, isolated from the M mask slots: gaps of the mask first, free slots after."""
    return [gap_hit(i) if i < M else slot(i) for i in range(first, first + H)]


class Case:
    def __init__(self, name, M, hits, expect, mtl=MTL, mdbr=0, at_end=False, mask=None, reps=1):
        self.name, self.mtl, self.mdbr, self.reps = name, mtl, mdbr, reps
        self.mask = [slot(i) for i in range(M)] if mask is None else mask
        self.hits = hits
        hi = max([e for _, e in hits] + [e for _, e in self.mask])
        self.lq = hi if at_end else hi + 3000
        self.expect = expect  # what the case is meant to reach, stated by construction: checked against the model
        # the records on T, one every `gap` bases, and the return windows' stretch of R
        self.gap = max(e - s for s, e in hits) + 10
        self.lt = 1000 + len(hits) * self.gap + 1000
        self.lr = max(r + w for _, w, r in self.returns()) + 500

    def kw(self, **more):
        return dict(dict(transitive=True, min_transitive_len=self.mtl, min_distance_between_ranges=self.mdbr), **more)

    def model(self, filter_covered=False):
        return model(self.mask, self.hits, self.lq, self.mtl, self.mdbr, filter_covered)

    # -- the PAF --
    def returns(self):
        """(a, w, r) of the windows Q[a, a + w) <-> R[r, r + w) that carry levels 2..4."""
        lo, hi = min(s for s, _ in self.hits), max(e for _, e in self.hits)  # (where the hits are: the mask may reach far beyond)
        nb = 6
        w = max(60, min(2500, (hi - lo) // (2 * nb)))
        w = min(w, hi - lo)
        return [(lo + j * (hi - lo - w) // (nb - 1), w, 500 + j * (w + 200)) for j in range(nb)]

    def paf(self):
        """(text, ranges as (sequence name, start, end)).  reps > 1: the H records are reps queries' ONE hit each -- H
        distinct ranges on T, each covering one record, the batch repeated reps times."""
        H = len(self.hits)
        G, lt, lr, win = self.gap, self.lt, self.lr, self.returns()
        lines = []
        for k, (s, e) in enumerate(self.hits):
            ts = 1000 + k * G
            lines.append("Q\t%d\t%d\t%d\t%s\tT\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%d=" %
                         (self.lq, s, e, "+-"[k % 2], lt, ts, ts + (e - s), e - s, e - s, e - s))
        for j, (a, w, r) in enumerate(win):
            lines.append("R\t%d\t%d\t%d\t+\tQ\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%d=" % (lr, r, r + w, self.lq, a, a + w, w, w, w))
            v = w - 20
            lines.append("Q\t%d\t%d\t%d\t%s\tR\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%d=" %
                         (self.lq, a + 13, a + 13 + v, "+-"[j % 2], lr, r + 7, r + 7 + v, v, v, v))
        if self.reps == 1:
            ranges = [("T", 500, lt - 500)]
        else:
            ranges = [("T", 1000 + k * G - 3, 1000 + k * G + 3) for k in range(H)] * self.reps
        return "\n".join(lines) + "\n", ranges

    def masked(self, seq_id):
        """masked_regions for the runs that give Q its old list (every sequence listed: one that is not gets length 0)."""
        return {seq_id("T"): (self.lt, []), seq_id("Q"): (self.lq, list(self.mask)), seq_id("R"): (self.lr, [])}


def disjoint(name, M, H, **expect):
    tier = tier_of(M + H, M)
    wave = tier in WAVE_CAP
    # (a lane's k-th isolated hit finds M + k - 1 ranges and k - 1 pieces, adds one of each: they meet when M + 2 H - 1 reaches the column)
    col = LANE_COL if tier == "lane" else MID_COL
    e = dict(cap=M + H, old=M, tier=tier, final_len=M + H, raw_pieces=H, pieces=H, leave=None, inplace=False,
             tiled=wave and H > WAVE_CAP[tier], spill=(not wave) and M + 2 * H - 1 >= col)
    e.update(expect)
    return Case(name, M, shuffled(fillers(M, H)), e)


def nests(name, M, n_nests, depth, far_mask=0, **expect):
    """n_nests centres, `depth` hits around each, every one three bases wider on either side than the one before: two
    pieces a hit (one for a nest's first, two if it sits on a mask range), dealt round-robin over the nests.  far_mask
    more mask ranges lie beyond the nests."""
    step = 3
    sp = 2 * step * depth + 40
    centre = lambda j: X0 + j * sp + step * depth
    mask = [(centre(j) - 2, centre(j) + 2) for j in range(M)] + [(X0 + n_nests * sp + 50 + i * 20, X0 + n_nests * sp + 60 + i * 20) for i in range(far_mask)]
    hits = [(centre(j) - 2 - step * k, centre(j) + 2 + step * k) for k in range(1, depth + 1) for j in range(n_nests)]
    old, H = M + far_mask, n_nests * depth
    raw = 2 * depth * min(M, n_nests) + (2 * depth - 1) * (n_nests - min(M, n_nests))
    tier = tier_of(old + H, old)
    e = dict(cap=old + H, old=old, tier=tier, final_len=max(M, n_nests) + far_mask, raw_pieces=raw,
             pieces=2 * min(M, n_nests) + (n_nests - min(M, n_nests)), leave=None, inplace=False,
             tiled=tier in WAVE_CAP and raw > WAVE_CAP[tier], spill=False)
    e.update(expect)
    return Case(name, 0, hits, e, mask=mask)


# insert semantics: (M, H) of one representative group per tier -- cap 8, 30, 100, 600, and old 900
REPRESENTATIVES = dict(lane=(4, 4), mid=(15, 15), tiny=(50, 50), small=(300, 300), large=(900, 60))


def variant(kind, tname):
    M, H = REPRESENTATIVES[tname]
    n = max(2, min(M, H) // 4 * 2)  # the slots the variant works on (an even number, half of what there is)
    base = dict(cap=M + H, old=M, tier=tname)
    name = "%s-%s" % (kind, tname)
    x = lambda i: slot(i)[0]
    y = lambda i: slot(i)[1]
    half = fillers(M, H - n, first=M if kind == "cover_all" else n)  # isolated hits beyond the slots the variant works on
    if kind == "touching":  # end == x, start == y: they extend the range; one base short: they do not
        hits = []
        for i in range(n):
            short = 1 if i % 4 >= 2 else 0
            hits.append((x(i) - 8 - short, x(i) - short) if i % 2 == 0 else (y(i) + short, y(i) + 8 + short))
        n_short = sum(1 for i in range(n) if i % 4 >= 2)
        return Case(name, M, shuffled(hits + half), dict(base, final_len=M + len(half) + n_short, raw_pieces=H, pieces=H))
    if kind == "duplicates":  # exact copies of list ranges: nothing new, nothing changes
        hits = [slot(i) for i in range(n)]
        return Case(name, M, shuffled(hits + half), dict(base, final_len=M + len(half), raw_pieces=len(half), pieces=len(half)))
    if kind == "cover_all":  # one hit over every range of the list: merge_forward_from runs to the end
        first = fillers(M, n - 1)  # (gaps of the mask: inside the big hit)
        big = (x(0) - 5, max(y(M - 1), max(e for _, e in first)) + 5)
        k = len(first) // 2
        hits = shuffled(first[:k]) + [big] + first[k:] + half  # (first[k:] come after the big hit: covered)
        return Case(name, M, hits, dict(base, final_len=1 + len(half), raw_pieces=k + (M + k + 1) + len(half)))
    if kind == "descending":
        hits = sorted(fillers(M, H), reverse=True)
        return Case(name, M, hits, dict(base, final_len=M + H, raw_pieces=H, pieces=H))
    if kind == "mdbr":  # gaps of mdbr - 1, mdbr, mdbr + 1 to the range before / behind: the first is dropped
        d, hits, kept = 20, [], 0
        for i in range(n):
            g = d - 1 + (i // 2) % 3
            hits.append((y(i) + g, y(i) + g + 8) if i % 2 == 0 else (x(i) - g - 8, x(i) - g))
            kept += g >= d
        return Case(name, M, hits + half, dict(base, final_len=M + kept + len(half), raw_pieces=kept + len(half)), mdbr=d)
    if kind == "mtl":  # pieces of exactly min_transitive_len and one base shorter, isolated and sticking out of a range
        t, hits, long_ = 8, [], 0
        for i in range(n):
            ln = t - (i // 2) % 2
            hits.append((x(i) + 40, x(i) + 40 + ln) if i % 2 == 0 else (y(i) - 3, y(i) + ln))
            long_ += ln >= t
        return Case(name, M, shuffled(hits + half), dict(base, final_len=M + n // 2 + len(half), raw_pieces=long_ + len(half)), mtl=t)
    if kind == "seq_end":  # the last mask range ends at the sequence's end; a hit reaches it, another starts the sequence
        hits = fillers(M, H - 2) + [(0, 30), (y(M - 1) - 45, y(M - 1))]
        return Case(name, M, shuffled(hits), dict(base, final_len=M + H - 1, raw_pieces=H), at_end=True)
    if kind == "covered":  # covered exactly; by the range before, ending exactly at its end; uncovered by one base on either side
        hits = []
        for i in range(n):
            hits.append([slot(i), (x(i) + 3, y(i)), (x(i) + 3, y(i) + 1), (x(i) - 1, y(i))][i % 4])
        unc = sum(1 for i in range(n) if i % 4 >= 2)
        return Case(name, M, shuffled(hits + half), dict(base, final_len=M + len(half), raw_pieces=unc + len(half)), mtl=1)
    raise KeyError(kind)


def touching_chain(name, M):
    """Behind every mask range two hits in a row, the first starting at the range's end, the second at the first's: both
    belong to the range (start == end of the one before, impg.rs:330-334), the list stays M ranges long.  A replay that
    fails to merge them keeps 3 M ranges -- with min_distance_between_ranges = 0 the same coverage and therefore the same
    rows at every later level; what differs is the LENGTH of the list, which level 3 finds as the group's old list: M is
    chosen so that the two lengths put that level's group on different tiers (tests assert the level-3 tier)."""
    hits = [h for i in range(M) for h in ((slot(i)[1], slot(i)[1] + 8), (slot(i)[1] + 8, slot(i)[1] + 16))]
    return Case(name, M, hits, dict(cap=3 * M, old=M, tier=tier_of(3 * M, M), final_len=M, raw_pieces=2 * M, pieces=M))


VARIANTS = ["touching", "duplicates", "cover_all", "descending", "mdbr", "mtl", "seq_end", "covered"]


def one_hit_each(name, M, reps, tier):
    """64 records, 64 x reps queries of one hit each against a mask of M ranges: 64 x reps groups of cap M + 1."""
    c = Case(name, M, fillers(M, 64), dict(cap=M + 1, old=M, tier=tier, groups=64 * reps), reps=reps)
    return c


def all_cases():
    cs = []
    # tier boundaries: cap = 12 | 13, 48 | 49, 128 | 129
    for M, H in [(0, 12), (3, 9), (0, 13), (6, 7), (10, 38), (24, 25), (0, 49), (64, 64), (0, 128), (64, 65), (0, 129)]:
        cs.append(disjoint("cap%d-old%d" % (M + H, M), M, H))
    # lane column collisions (list + pieces beyond the 12- / 64-entry column) and their neighbours that fit
    cs.append(disjoint("column12-collide", 6, 6, spill=True))
    cs.append(disjoint("column12-fits", 6, 3))
    cs.append(disjoint("column64-collide", 24, 24, spill=True))
    cs.append(disjoint("column64-fits", 24, 8))
    # wave small | large by the old length
    cs.append(disjoint("old832", 832, 5))
    cs.append(disjoint("old833", 833, 5))
    # large tier: the last list that is loaded into LDS, the first that never is
    cs.append(disjoint("old4032", 4032, 40))
    cs.append(disjoint("old4033", 4033, 40, leave=0, inplace=True))
    # outgrowing the small buffer (a batch of 64 needs room: 1 152 isolated hits fit, the 1 153rd does not)
    cs.append(disjoint("grow1151", 0, 1151))
    cs.append(disjoint("grow1152", 0, 1152))
    cs.append(disjoint("grow1153", 0, 1153, leave=1152, inplace=True))
    cs.append(disjoint("grow1400", 0, 1400, leave=1152, inplace=True))
    cs.append(disjoint("grow800+400", 800, 400, leave=320, inplace=True))
    cs.append(disjoint("grow800+288", 800, 288))
    # ... and the large one
    cs.append(disjoint("grow4000+200", 4000, 200, leave=64, inplace=True))
    cs.append(disjoint("grow4000+32", 4000, 32))
    # more pieces than the buffer, the list staying small: the tiled sort alone, per tier, with a neighbour just under
    cs.append(nests("tiled-tiny", 0, 8, 13))          # 8 x 25 = 200 pieces > 192, cap 104
    cs.append(nests("untiled-tiny", 0, 8, 12))        # 8 x 23 = 184
    cs.append(nests("tiled-small", 0, 40, 15))        # 40 x 29 = 1 160 > 1 152
    cs.append(nests("untiled-small", 0, 40, 14))      # 40 x 27 = 1 080
    cs.append(nests("tiled-large", 100, 100, 21, far_mask=800))    # 100 x 42 = 4 200 > 4 096, old 900
    cs.append(nests("untiled-large", 100, 100, 20, far_mask=800))  # 4 000
    # the pre-pass moves a group across a boundary: 49 -> 48 (tiny -> mid) with one covered hit
    cs.append(Case("covered-49-to-48", 24, shuffled(fillers(24, 24) + [slot(5)]), dict(cap=49, old=24, tier="tiny", final_len=48, raw_pieces=24, pieces=24)))
    # touching hits that must merge, seen through the tier level 3 takes: 20 | 60 ranges (mid | tiny), 420 | 1 260 (small | large)
    cs.append(touching_chain("touching-chain-tiny", 20))
    cs.append(touching_chain("touching-chain-small", 420))
    for kind in VARIANTS:
        for tname in REPRESENTATIVES:
            cs.append(variant(kind, tname))
    # lists longer than one round of their grid
    cs.append(one_hit_each("many-lane", 5, TINY_GRID // 64 + 1, "lane"))
    cs.append(one_hit_each("many-tiny", 48, TINY_GRID // 64 + 1, "tiny"))  # 8 256 groups > 8 192 blocks
    cs.append(one_hit_each("many-mid", 12, MID_GRID // 64 + 1, "mid"))     # 81 984 groups > 1 280 blocks x 64 lanes
    return cs


CASES = {c.name: c for c in all_cases()}
assert len(CASES) == len(all_cases())
