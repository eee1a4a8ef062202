"""Inputs for the per-query walk's MultiImpg arm (walk_device.inc, walk_body<.., MULTI>): what tests/dfs_gen.py cannot reach with
its one-op alignments, min_distance_between_ranges = 0 and min_transitive_len <= 1.

The fixtures are PAF text only -- never an expected output: that is the oracle's (oracle/impg_oracle.cpp, multi_transitive).
tests/test_multi_walk_gen_cpu.py shows on the CPU that each one reaches the edge it was built for; tests/test_gpu_walk_multi.py
runs them on the walk, at both ends of the worklist.

As in dfs_gen every index is built with bidirectional=False, so `edge(src, ss, dst, ds, ..)` is a one-way step from src to dst;
sequence ids are given in order of first appearance, a line's query name first, and `id_order` lines (at FAR, reached by no
query) fix that order.  Every fixture is a graph without cycles (a sequence's copies onto itself aside, which the worklist
skips): a wrong engine fails, it does not spin.
"""
import re

from tests import dfs_gen as dg
from tests import walk_gen as wg
from tests.paf_gen import random_paf, random_ranges

SEQ_LEN = wg.SEQ_LEN
FAR = dg.FAR
id_order = dg.id_order
POP_BUDGET = 1 << 20  # WALK_POP_BUDGET (walk_device.inc); pinned to the source by the CPU test


def spans(cigar):
    ops = [(int(n), c) for n, c in re.findall(r"(\d+)([=XIDM])", cigar)]
    return sum(n for n, c in ops if c in "=XDM"), sum(n for n, c in ops if c in "=XIM"), ops


def edge(src, ss, dst, ds, cigar=100, strand="+"):
    """one PAF line: target src from ss, query dst from ds; cigar: a CIGAR string, or the length of one `=` op"""
    if isinstance(cigar, int):
        cigar = "%d=" % cigar
    td, qd, _ = spans(cigar)
    return "%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%s\n" % (dst, SEQ_LEN, ds, ds + qd, strand, src, SEQ_LEN, ss, ss + td, td, max(td, qd), cigar)


def op_cuts(cigar, ts):
    """target positions at which an op of the alignment starts or ends"""
    at, out = ts, {ts}
    for n, c in spans(cigar)[2]:
        if c in "=XDM":
            at += n
        out.add(at)
    return out


def P(depth, **kw):
    """a parameter set (the end of the worklist, `dfs`, is the test's to choose)"""
    return dict(dict(transitive=True, multi_impg=True, max_depth=depth, min_transitive_len=1, min_distance_between_ranges=0), **kw)


class Fixture:
    """texts: one PAF text per alignment file.  queries: (name, start, end).  kws: parameter sets, each run at both ends.
    keep: names the subset filter keeps (None: no filter)."""

    def __init__(self, name, texts, queries, kws, keep=None):
        self.name, self.texts, self.queries, self.kws, self.keep = name, texts, queries, kws, keep


def files(lines, n_files, head):
    return dg.split(lines, n_files, head)


# ---- proximity: reverse-strand hits 9 and 10 bases from a visited range, on each side ----------------------------------------
PROX_ORDER = ["T", "X", "Y", "W"]


def proximity():
    """T:[0, 100) -> X:[1000, 1100) and Y:[0, 100).  Y:[0, 100) has four reverse-strand images on X, in the order of their
    q_first (the larger coordinate): D [890, 990) 10 below the visited range, C [891, 991) 9 below, A [1109, 1209) 9 above, B
    [1110, 1210) 10 above.  Under min_distance_between_ranges = 10: D and B are inserted and expanded, C and A are reported and
    nothing else.  X:[800, 1300) -> W + 5000 shows what was expanded: W rows of [890, 990), [1000, 1100), [1110, 1210) exactly
    (an inserted C would lengthen D's record to [890, 991), an inserted A B's to [1109, 1210))."""
    lines = id_order(PROX_ORDER)
    lines += [edge("T", 0, "X", 1000), edge("T", 0, "Y", 0)]
    lines += [edge("Y", 0, "X", at, 100, "-") for at in (1109, 890, 1110, 891)]
    lines += [edge("X", 800, "W", 5800, 500)]
    return files(lines, 2, len(id_order(PROX_ORDER)))


# ---- pieces of 100 and 101 bases under min_transitive_len = 101 ---------------------------------------------------------------
def piece_lengths():
    """T:[0, 300) -> X:[0, 100) (a piece of 100: reported, not pushed) and Z:[0, 101) (pushed); X -> W:[0, 100), Z -> W:[1000, 1101)"""
    lines = id_order(["T", "X", "Z", "W"])
    lines += [edge("T", 0, "X", 0, 100), edge("T", 150, "Z", 0, 101), edge("X", 0, "W", 0, 100), edge("Z", 0, "W", 1000, 101)]
    return files(lines, 2, 2)


# ---- a hit on the popped sequence itself ----------------------------------------------------------------------------------------
def self_hit():
    """T:[0, 100) -> S:[0, 100); S:[0, 100) -> S:[500, 600), a record whose query and target are one sequence, met at depth 1;
    S:[500, 600) -> V.  MultiImpg: the hit is in no row and expands nothing.  Plain DFS reports it (and expands nothing either)."""
    lines = id_order(["T", "S", "V", "U"])
    lines += [edge("T", 0, "S", 0), edge("S", 0, "S", 500), edge("S", 500, "V", 0), edge("S", 0, "U", 0)]
    return lines


# ---- I / D / X ops cut by the popped range -----------------------------------------------------------------------------------------
INDEL_T = "30=10I20=7D15X28="        # T from 100: ops end at 130, 130, 150, 157, 172, 200
INDEL_X = "12=5D9X6I40=3D25="        # X from 1000
INDEL_QUERY = ("T", 140, 165)        # cuts the 20= and the 15X


def indels():
    """T:[140, 165) starts inside an `=` op and ends inside an `X` op of T -> X (both strands, two files); the pieces it leaves on X
    start and end inside ops of X -> W.  Every later pop is cut the same way."""
    lines = id_order(["T", "X", "W", "V"])
    lines += [edge("T", 100, "X", 1000, INDEL_T), edge("T", 100, "X", 3000, INDEL_T, "-"), edge("X", 1000, "W", 0, INDEL_X),
              edge("X", 2990, "W", 500, INDEL_X, "-"), edge("W", 0, "V", 0, "20=4I30=2D600=")]
    return files(lines, 2, 2)


# ---- entries that only touch the popped range ------------------------------------------------------------------------------------------
def touching():
    """T:[0, 100) -> Y:[100, 200).  On Y: an entry that ends where the range starts ([50, 100) -> A), one that starts where it ends
    ([200, 250) -> B), one inside ([120, 170) -> C).  The closed test looks all three up; what comes of the two is the oracle's."""
    lines = id_order(["T", "Y", "A", "B", "C"])
    lines += [edge("T", 0, "Y", 100), edge("Y", 50, "A", 0, 50), edge("Y", 200, "B", 0, 50), edge("Y", 120, "C", 0, 50)]
    return files(lines, 2, 3)


# ---- ties on the first one, two, three and four sort keys -----------------------------------------------------------------------
def ties():
    """T:[0, 1000) -> Y:[0, 1000); the pop of Y, at depth 1, has hits on Q that agree on
      1 key   (Q)                               Q:[7000, 7100) from Y:[600, 700)
      2 keys  (Q, 5000)                         Q:[5000, 5150) from Y:[100, 250)
      3 keys  (Q, 5000, 5100)                   from Y:[300, 400) and from Y:[100, 200)
      4 keys  (Q, 5000, 5100, 100)              from Y:[100, 210), `50=10D50=`, and from Y:[100, 200)
    spread over three files so that the files' order is not the sorted one.  Q -> R shows the replay.  (Hits that agree on all five
    keys are identical rows: without store_cigar their order is invisible, and the walk declines store_cigar.)"""
    head = id_order(["T", "Y", "Q", "R"])
    f0 = head + [edge("T", 0, "Y", 0, 1000), edge("Y", 600, "Q", 7000), edge("Y", 100, "Q", 5000, "50=10D50=")]
    f1 = [edge("Y", 300, "Q", 5000), edge("Y", 100, "Q", 5000, 150)]
    f2 = [edge("Y", 100, "Q", 5000), edge("Q", 4000, "R", 0, 4000)]
    return ["".join(f0), "".join(f1), "".join(f2)]


# ---- the front pop's cursor ---------------------------------------------------------------------------------------------------------
PADS = 70
FRONT_ORDER = ["D1", "E", "D2", "X", "T", "M"] + ["p%d" % i for i in range(PADS)] + ["Z", "ZZ", "W"]


def front_cursor():
    """max_depth 2, popped at the front.  T -> E, X:[200, 300), M, Z (depth 1).  E, the lowest, goes first: D1, D2, X:[0, 100) and
    X:[400, 500) at depth 2.  The next pop drops D1's and D2's lists whole (the cursor moves up twice), drops X:[0, 100) in front
    of the explorable X:[200, 300) and leaves X:[400, 500) behind it: the list then starts two records in.  The pop after drops that
    one and explores M -> D1:[500, 600) and ZZ (depth 2).  Then D1's list is dropped and the cursor must pass X, T, M and 70
    sequences that never had a record to find Z: two looks of 64.  X -> W shows which records of X were explored: [200, 300) only."""
    lines = id_order(FRONT_ORDER)
    head = len(lines)
    lines += [edge("T", 0, "E", 0), edge("T", 0, "X", 200), edge("T", 0, "M", 0), edge("T", 0, "Z", 0)]
    lines += [edge("E", 0, "D1", 0), edge("E", 0, "D2", 0), edge("E", 0, "X", 0), edge("E", 0, "X", 400)]
    lines += [edge("M", 0, "D1", 500), edge("M", 0, "ZZ", 0), edge("Z", 0, "ZZ", 1000), edge("X", 0, "W", 0, 600)]
    return files(lines, 2, head)


# ---- the subset filter ---------------------------------------------------------------------------------------------------------------
SUBSET_KEEP = ["C", "B", "G"]


def subset():
    """keep = {C, B, G}: T, the original target, is not kept.  T -> A -> G: A is dropped, so G is never reached through it.  T -> C
    -> T:[5000, 5100): a hit on the original target passes although keep[T] is 0, and leads on, T:[5000, 5100) -> B."""
    lines = id_order(["T", "A", "C", "B", "G"])
    lines += [edge("T", 0, "A", 0), edge("A", 0, "G", 0), edge("T", 0, "C", 0), edge("C", 0, "T", 5000), edge("T", 5000, "B", 0)]
    return files(lines, 2, 3)


# ---- min_output_length, min_identity ---------------------------------------------------------------------------------------------------
def output_length():
    """min_output_length 100.  T:[0, 200) -> X:[0, 50): too short for a row, still replayed and pushed; X:[0, 50) -> W with
    `25=100I25=`, 150 bases of W: a row that only an expanded X explains.  T:[0, 200) -> Z:[0, 150) is a row."""
    lines = id_order(["T", "X", "Z", "W"])
    lines += [edge("T", 0, "X", 0, 50), edge("T", 50, "Z", 0, 150), edge("X", 0, "W", 0, "25=100I25=")]
    return files(lines, 2, 2)


def identity():
    """min_identity 0.8: T -> X with `90=10X` (0.9) is a hit, T -> Z with `50=50X` (0.5) is none; each leads one step on"""
    lines = id_order(["T", "X", "Z", "W", "V"])
    lines += [edge("T", 0, "X", 0, "90=10X"), edge("T", 0, "Z", 0, "50=50X"), edge("X", 0, "W", 0), edge("Z", 0, "V", 0)]
    return files(lines, 2, 3)


_fixtures = [
    Fixture("proximity", proximity(), [("T", 0, 100)], [P(0, min_distance_between_ranges=10), P(3, min_distance_between_ranges=10)]),
    Fixture("piece-lengths", piece_lengths(), [("T", 0, 300)], [P(0, min_transitive_len=101), P(0, min_transitive_len=100)]),
    Fixture("self-hit", ["".join(self_hit())], [("T", 0, 100)], [P(0), P(2)]),
    Fixture("indels", indels(), [INDEL_QUERY, ("T", 100, 200), ("X", 1010, 1030)], [P(0), P(2), P(0, min_transitive_len=5, min_distance_between_ranges=3)]),
    Fixture("touching", touching(), [("T", 0, 100), ("Y", 100, 200)], [P(0), P(1)]),
    Fixture("ties", ties(), [("T", 0, 1000), ("Y", 0, 1000)], [P(0), P(2)]),
    Fixture("front-cursor", front_cursor(), [("T", 0, 100)], [P(2), P(3), P(0)]),
    Fixture("subset", subset(), [("T", 0, 100)], [P(0), P(2)], keep=SUBSET_KEEP),
    Fixture("output-length", output_length(), [("T", 0, 200)], [P(0, min_output_length=100), P(0)]),
    Fixture("identity", identity(), [("T", 0, 100)], [P(0, min_identity=0.8), P(0)]),
]
FIXTURES = {f.name: f for f in _fixtures}


# ---- a random index with cycles, both strands and indels (built with bidirectional=True) ------------------------------------------
RANDOM_SEQS, RANDOM_LEN, RANDOM_FILES, RANDOM_RANGES = 7, 40_000, 3, 128


def random_texts():
    """about 600 records over 7 sequences of 40 kb in three files (tests/paf_gen.py: random CIGARs of all five ops, both strands,
    records of a sequence onto itself)"""
    return [random_paf(4100 + k, 200, n_seq=RANDOM_SEQS, seq_len=RANDOM_LEN, max_ops=150, weird=(k == 1), self_aln=True)[0] for k in range(RANDOM_FILES)]


def random_queries():
    """128 ranges of 1 to 5 000 bases, as (sequence name, start, end)"""
    return [("s%d" % t, s, e) for t, s, e in random_ranges(4177, RANDOM_RANGES, RANDOM_SEQS, RANDOM_LEN, max_len=5000, min_len=1)]


RANDOM_KEEP = ["s0", "s2", "s3", "s6"]
# (kw, subset filter or not); each run at both ends
RANDOM_KWS = [
    (P(2, min_transitive_len=30), False),
    (P(0, min_transitive_len=101, min_distance_between_ranges=10), False),
    (P(3, min_transitive_len=30, min_distance_between_ranges=40, min_output_length=200), False),
    (P(0, min_transitive_len=101, min_identity=0.6), False),
    (P(3, min_transitive_len=30, min_distance_between_ranges=10), True),
]


# ---- the slab's limits under MultiImpg semantics (tests/walk_gen.py has the capacities and the arithmetic) ----------------------------
# pairs of one step (bit 2): walk_gen's pile.  The closed test and the self-skip change nothing: every entry of T is T:[1000, 1100),
# none merely touches it, none maps T onto itself.  max_depth 1: the pieces on Q are dropped in one step (the batch engine that
# answers the falling side then takes two rounds, not 4 097).
PAIRS_STAYS, PAIRS_FALLS = 4096, 4097
PAIRS_KW = P(1)
# the stack pool (bit 32): walk_gen's spread.  The pop of T opens n lists of max(8, 2 k) = 8 records beside T's own 8, the pop of W
# n more: 8 + 16 n against scap = 65 536 -- 4 095 stays (65 528), 4 096 falls (65 544).  Popped at the back, as walk_gen's S-stack.
STACK_STAYS, STACK_FALLS = 4095, 4096
STACK_KW = P(2)


def stack_use(n):
    return 8 + 2 * n * 8
