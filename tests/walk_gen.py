"""Inputs that put one query of the per-query walk (impg_amd/csrc/walk_device.inc, Engine::run_walk) on either side of every
limit of its slab, and the arithmetic that says which side.

A workgroup owns a query inside a fixed slab of HBM.  When the query outgrows the slab the kernel raises a cause bit,
run_walk returns false and the batch engine answers: counter "walk_overflow" is that word for the last launch.  The fixtures
here are PAF text and mask lists only -- never an expected output: that is the oracle's.

Every alignment is one `100=` op unless a length is given; every index is built with bidirectional=False, so a pile has no
way back and deeper levels cost nothing.  All fixtures carry a small side component (U <-> V) for the "next ordinary query".

The giant piles are built with ORDER_SORTED (and the oracle's sorted policy): the hits of one window then come in input
order, their images ascending on the query sequence, so the one thread that replays a (query, sequence) group appends at the
list's end.  In the reference's tree order the same replay shifts half the list per hit: 10^8 moves for 32 767 hits, by one
thread.  The fan of case D (1 000 hits a range) runs in the reference's order.

The limits (Engine::walk_caps; pinned to the source by tests/test_walk_gen_cpu.py):

    form                         wcap     hcap     vcap      gcap     scap
    wave (DFS, one wave)         4 096    4 096    131 072   16 384   65 536
    wide (BFS, 16 waves; grid)   16 384   32 767   131 072   262 144  16

and pairs per step < 2^15 (WALK_SLOT_BITS), a row region of 2^17 rows per query for batches of <= 64 ranges (else none:
count first, then place).

Which limit fires first, per cause bit:

  1   unknown target.  Reachable, whatever the issue supposed: check_ranges looks at start < end only, and a query on an id
      the index does not hold is a valid one (its own row comes back, impg.rs:1896).  The walk raises 1 before it touches
      anything and the batch engine answers.  No case here yet: the oracle's tables have no entry for such an id, so the
      expected rows would have to be written out; every case asserts that its own query does not raise it.
  2   pairs of one step (P > hcap, P >= 2^15) or of one member's share of the last level (P > hcap).  Cases A, B, E, E'.
      A level of several ranges is first cut (sub halves) down to one range per step: only a single range's window can
      raise it outside the grid's last level -- case D is the cut that does not raise it.
  4   a mask list that does not fit (mlen + 1 > wcap is the binding term: 2 (mlen + 1) <= vcap and mlen + 1 <= gcap, scap
      hold whenever it does) -- case H; or the visited pool (lists move to 2 (len + n) slots and abandon their old place)
      -- case V.  The issue's candidate, fan_disjoint(2, 30000), does not reach it, for two reasons found by running it:
      level 2's first sub-step yields 30 000 pieces of length 100 > wcap, so 16 fires first; and with the pieces out of the
      way the walk stays -- a list moves only when len + n > cap, and the second sub-step's 30 000 + 30 000 is exactly the
      2 (0 + 30 000) slots the first one took.  V makes the first hop 300 long and sets min_transitive_len 200 (R's images,
      100 long, lengthen its list and leave no piece) and has three places of 20 000: R's list takes 2 (0 + 20 000) slots,
      holds the second place's hits in them (40 000 <= 40 000), and moves at the third to 2 (40 000 + 20 000) behind the
      16 + 40 000 already used: 160 016 > 131 072.
  8   piece scratch: a step's groups take len + 2 n slots of gcap each.
      wide: unreachable.  Sum n <= P <= 32 767, and every list lives in the pool, so Sum len <= vcap (a group that does not
      fit the pool raises 4 and takes no scratch): 131 072 + 65 534 = 196 606 <= 262 144.
      wave: reachable, 4 096 pairs a pop give 8 192, so a list of more than 8 192 ranges that is hit 4 096 times again does
      it: case G, fan_disjoint(4, 4000), DFS depth 2 -- R's list is 0, 4 000, 8 000 and 12 000 long at the four pops of Q's
      places: 12 000 + 8 000 = 20 000 > 16 384 (the third, 8 000 + 8 000 = 16 000, fits); its pool use, 8 000 + 16 000 +
      24 000, stays below vcap.  (First hop 300 long and min_transitive_len 200, as in V: no piece of R goes on the stack --
      the batch engine's DFS, a round of launches per pop, would spend seconds on dropping 16 000 of them.)
  16  pieces of one level / pop (npc > wcap).  BFS: case C's falling side -- see 32.  DFS: a pop has <= 4 096 hits and wcap
      is 4 096, so only hits that leave several pieces each could do it; C covers the comparison.
  32  BFS frontier (n_new > wcap): unreachable.  The frontier is the merged pieces, n_new <= npc, and npc > wcap has raised
      16 in the update already.  The issue names 32 for case C's falling side; what the code raises at n = 16 385, and all
      it can raise, is 16.  C asserts 16 and that 32 is absent.
      DFS stack pool (scap records; a sequence's first push takes max(8, 2 k)): case S, spread(4096) -- a pop of T hits W and
      4 095 sequences once each, the pop of W 4 096 more: 8 (T) + 4 096 x 8, then 4 096 x 8 more = 65 544 > 65 536.  The
      visited pool holds the same 8 slots per sequence (65 544 + 8 <= 131 072) and the scratch 2 per group.
  64  unnamed: must never be seen.  (The grid's leader reports its own share's 2 alone: E and E' would show a 64 beside it.)
  128 a grid hand-off timed out: never provoked here, only asserted absent.
"""
WAVE = dict(wcap=4096, hcap=4096, vcap=131072, gcap=16384, scap=65536)
WIDE = dict(wcap=16384, hcap=32767, vcap=131072, gcap=262144, scap=16)
SLOT_BITS = 15          # pairs per step < 2^15
ROW_REGION = 1 << 17    # rows a query may write in the first pass (batches of <= SMALL_RANGES ranges)
SMALL_RANGES = 64
UNKNOWN, PAIRS, POOL, SCRATCH, PIECES, STACK = 1, 2, 4, 8, 16, 32
NEVER = 1 | 64 | 128    # bits no case may show beside its own
SEQ_LEN = 80_000_000    # (a pile of 32 768 images 2 000 apart ends at 65.5 Mbp)
PLACE_STEP = 10_000     # fan: the places on Q
R_TO_S = 200            # fan: alignments from R on to S


def aln(q, qs, t, ts, n=100, strand="+"):
    """one PAF line: query q:[qs, qs + n) on target t:[ts, ts + n), CIGAR `n=`"""
    return "%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%d=\n" % (q, SEQ_LEN, qs, qs + n, strand, t, SEQ_LEN, ts, ts + n, n, n, n)


def side():
    """a small component of its own: the "next ordinary query" is (U, 0, 2000)"""
    return [aln("V", 1000, "U", 100, 500), aln("V", 4000, "U", 300, 400, "-"), aln("U", 5000, "V", 1200, 300),
            aln("V", 9000, "U", 5100, 150), aln("U", 7000, "V", 9020, 120, "-")]


SIDE_RANGE = ("U", 0, 2000)
SIDE_KW = dict(max_depth=3, min_transitive_len=10, min_distance_between_ranges=0)
PILE_RANGE = ("T", 1000, 1100)


def pile(n):
    """n alignments of T:1000-1100, the k-th to Q:[2000 k, +100): one range, one window of exactly n hits, n pieces"""
    return "".join([aln("Q", 2000 * k, "T", 1000) for k in range(n)] + side())


def fan(places, per, image_step=None, first_len=100, last_place_first=False):
    """T:1000-(1000 + first_len) maps to `places` places on Q, PLACE_STEP apart; on each place a pile of `per` alignments from
    Q (the place's first 100 bases) to R, image j of place k at R:[70 j + k, +100) -- images overlap across places, strands
    alternate -- or, with image_step, image_step apart and all distinct (fan_disjoint).  R_TO_S alignments go from R on to S,
    spread over the span of the images, so a third level has work."""
    lines = [aln("Q", PLACE_STEP * k, "T", 1000, first_len) for k in range(places)]
    for k in range(places):
        for j in range(per):
            at = 70 * j + k if image_step is None else image_step * ((places - 1 - k if last_place_first else k) * per + j)
            lines.append(aln("R", at, "Q", PLACE_STEP * k, 100, "+-"[(j + k) & 1]))
    span = fan_span(places, per, image_step)
    gap = max(100, (span - 100) // R_TO_S)
    lines += [aln("S", 1000 * i, "R", gap * i) for i in range(R_TO_S)]
    return "".join(lines + side())


def fan_span(places, per, image_step=None):
    return (70 * (per - 1) + places - 1 if image_step is None else image_step * (places * per - 1)) + 100


def fan_disjoint(places, per, first_len=100, last_place_first=False):
    """the fan with images 200 apart on R: every hit lengthens R's visited list.  The images ascend on R in the order the
    hits are replayed, so that each one appends: place by place for a BFS; for a DFS, which pops Q's last place first,
    last_place_first puts that place's images first (the other way round every hit of the later pops shifts the whole list:
    4 000 x 8 000 moves by one lane, seconds)."""
    return fan(places, per, image_step=200, first_len=first_len, last_place_first=last_place_first)


def spread(n):
    """T:1000-1100 hits n - 1 sequences X0 .. and W once each; W:[0, 100) hits n more sequences Y0 ..: two pops of a DFS
    that open 2 n stack lists of one record (whichever of W and the Xs is popped first)."""
    lines = [aln("X%d" % k, 0, "T", 1000) for k in range(n - 1)]
    lines += [aln("W", 0, "T", 1000)]
    lines += [aln("Y%d" % k, 0, "W", 0) for k in range(n)]
    return "".join(lines + side())


def mask_list(m, first=2000, step=20, width=10):
    """m disjoint non-empty ranges [first + step i, + width): one target's list of a masked_regions map (random_mask's format:
    {sequence id: (sequence_length, [(start, end), ...])})"""
    return [(first + step * i, first + step * i + width) for i in range(m)]


MASK_RANGE = ("T", 0, 400_000)  # covers every range of mask_list(16 384): m + 1 self pieces


class Case:
    """One fixture on one side of one limit.  value / cap: the number the kernel compares and what it compares it with
    (value <= cap: stays).  `bit`: the cause expected on the falling side (0: stays).  kws: the query parameter sets (every
    one transitive); options: walk_kernel / walk_members.  order: "sorted" | "coitrees"."""

    def __init__(self, name, fixture, args, value, cap, bit, kws, options, dfs=False, order="sorted", mask=0, rng=PILE_RANGE, note=""):
        self.name, self.fixture, self.args, self.value, self.cap, self.bit = name, fixture, args, value, cap, bit
        self.kws, self.options, self.dfs, self.order, self.mask, self.range, self.note = kws, options, dfs, order, mask, rng, note
        assert (value <= cap) == (bit == 0), name

    def text(self):
        return self.fixture(*self.args)

    def params(self, kw):
        return dict(transitive=True, dfs=self.dfs, **kw)


BASE = dict(min_transitive_len=1, min_distance_between_ranges=0)  # every piece is kept, whatever is left of an image; no proximity test
ONE_WG = dict(walk_kernel=2, walk_members=1)   # every small BFS on one workgroup
GRID2 = dict(walk_kernel=1, walk_members=2)
GRID5 = dict(walk_kernel=1, walk_members=5)
DFS_OPT = dict(walk_kernel=1, walk_members=0)


def d(depth, **kw):
    return dict(max_depth=depth, **dict(BASE, **kw))


_cases = [
    # A  a DFS pop's pairs against hcap (wave): `P > A.hcap`
    Case("A-stays", pile, (4096,), 4096, WAVE["hcap"], 0, [d(2)], DFS_OPT, dfs=True),
    Case("A-falls", pile, (4097,), 4097, WAVE["hcap"], PAIRS, [d(2)], DFS_OPT, dfs=True),
    # B  one range's pairs against hcap (wide) and 2^15: `P > A.hcap || P >= (1u << WALK_SLOT_BITS)`.  The level is the last
    #    one (max_depth 1: no update).  With max_depth 0 the update runs and 32 767 pieces outgrow wcap: B0 shows that the
    #    32 767-hit group is replayed and reported as 16; at 32 768 the step check comes first under either depth.
    Case("B-stays", pile, (32767,), 32767, min(WIDE["hcap"], (1 << SLOT_BITS) - 1), 0, [d(1)], ONE_WG),
    Case("B-falls", pile, (32768,), 32768, min(WIDE["hcap"], (1 << SLOT_BITS) - 1), PAIRS, [d(1), d(0)], ONE_WG),
    Case("B0-pieces", pile, (32767,), 32767, WIDE["wcap"], PIECES, [d(0)], ONE_WG, note="B under max_depth 0: C's limit is met first"),
    # C  a level's pieces against wcap: `dst + np > A.wcap` (and the dead `n_new > A.wcap` behind it)
    Case("C-stays", pile, (16384,), 16384, WIDE["wcap"], 0, [d(3), d(0)], ONE_WG),
    Case("C-falls", pile, (16385,), 16385, WIDE["wcap"], PIECES, [d(3), d(0)], ONE_WG, note="the issue names 32: unreachable, see above"),
    # E  a member's share of the last level against hcap: `P + tot > A.hcap` in walk_final_level
    Case("E-stays", fan, (2, 32767), 32767, WIDE["hcap"], 0, [d(2)], GRID2),
    Case("E-falls", fan, (2, 32768), 32768, WIDE["hcap"], PAIRS, [d(2)], GRID2),
    Case("E'-stays", fan, (140, 1000), 140 // 5 * 1000, WIDE["hcap"], 0, [d(2)], GRID5),
    Case("E'-falls", fan, (140, 1000), 140 // 2 * 1000, WIDE["hcap"], PAIRS, [d(2)], GRID2),
    # H  a target's mask list against wcap: `mlen + 1u > A.wcap`.  Staying: min_transitive_len 5 keeps every self piece (10
    #    bases), the frontier / the stack open with exactly wcap records.  Falling: the same limit whatever the pieces'
    #    lengths; min_transitive_len 50 keeps the batch engine's DFS (a round of launches per pop) to a few pops.
    Case("H-dfs-stays", pile, (50,), 4095 + 1, WAVE["wcap"], 0, [d(2, min_transitive_len=5)], DFS_OPT, dfs=True, mask=4095, rng=MASK_RANGE),
    Case("H-dfs-falls", pile, (50,), 4096 + 1, WAVE["wcap"], POOL, [d(2, min_transitive_len=50)], DFS_OPT, dfs=True, mask=4096, rng=MASK_RANGE),
    Case("H-bfs-stays", pile, (50,), 16383 + 1, WIDE["wcap"], 0, [d(2, min_transitive_len=5)], ONE_WG, mask=16383, rng=MASK_RANGE),
    Case("H-bfs-falls", pile, (50,), 16384 + 1, WIDE["wcap"], POOL, [d(2, min_transitive_len=5)], ONE_WG, mask=16384, rng=MASK_RANGE),
    # V  the visited pool (see 4 above): 16 + 40 000 + 120 000 slots
    Case("V-pool", fan_disjoint, (3, 20000, 300), 16 + 2 * 20000 + 2 * 60000, WIDE["vcap"], POOL,
         [d(3, min_transitive_len=200)], ONE_WG, rng=("T", 1000, 1300)),
    # G  the wave form's piece scratch (see 8 above)
    Case("G-scratch", fan_disjoint, (4, 4000, 300, True), 3 * 4000 + 2 * 4000, WAVE["gcap"], SCRATCH,
         [d(2, min_transitive_len=200)], DFS_OPT, dfs=True, rng=("T", 1000, 1300)),
    # S  the DFS stack pool (see 32 above)
    Case("S-stack", spread, (4096,), 8 + 2 * 4096 * 8, WAVE["scap"], STACK, [d(2)], DFS_OPT, dfs=True),
]
CASES = {c.name: c for c in _cases}

# D and F stay, whatever the form: a level of more pairs than a step holds is cut (D), a query of more rows than its region is
# walked twice (F).  kws of D: the plain one, no depth limit, and a proximity test with a length cut-off under which the order
# of a level's hits shows in the pieces (a hit within 40 of a range already there is dropped, remainders under 30 are no pieces:
# 261 rows on S in the reference's visit order, 283 in ascending order, 200 without the two cut-offs).
D_FAN, F_FAN = (40, 1000), (140, 1000)
D_KWS = [d(3), d(0), d(3, min_distance_between_ranges=40, min_transitive_len=30)]
D_FORMS = dict(single=ONE_WG, grid2=dict(walk_kernel=2, walk_members=2), grid5=dict(walk_kernel=2, walk_members=5))
D_ROWS, F_ROWS = 1 + 40 + 40 * 1000 + R_TO_S, 1 + 140 + 140 * 1000   # d(3) / d(2)
F_KWS = [d(2), d(3)]
F_FORMS = dict(single=ONE_WG, grid5=GRID5)
assert 40 * 1000 > WIDE["hcap"] >= 20 * 1000 and F_ROWS > ROW_REGION and 140 // 5 * 1000 <= WIDE["hcap"]
