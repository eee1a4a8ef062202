"""Inputs that put a lookup window on a chosen path of the wide-window emit (kernels.hip: lookup_count_lane_kernel's wide
predicate, lookup_emit_wide_kernel's single pass / rank-bin groups / overflow list), and a plain model that says which path
each window takes.

The model restates, from (lo, ub, the visit ranks of the window's hits, order policy, max_seg, cap, bins):
  is_wide      a window [lo, ub) leaves the lane kernels iff ub - (lo & ~3) > 64 (the hit mask starts at the aligned entry).
               lo and ub are places in the index's one entry array, where the segments lie unpadded in sequence-id order
               (seg_offset: T first, T2 behind its n entries) -- so the boundary moves with (offset + lo) & 3;
  key_domain   the sort keys of its hits lie below dom = max_seg (ORDER_COITREES: the rank column) or ub - lo (ORDER_SORTED:
               the hit's place in the window);
  bin_shift    the smallest shift that puts every key below dom into a bin below `bins`;
  emit_plan    H <= cap hits: one pass; else the histogram of the hits' bins -- a bin of more than cap hits: the overflow list
               (lookup_emit_kernel); else bins gathered greedily into groups of at most cap hits, one pass per group.
It is used only to say what an input reaches (the lookup_wide_* counters of tests/test_gpu_lookup_paths.py) -- never as the
expected output of a query: that is the oracle's.

Where a rank comes from.  Under ORDER_COITREES an entry's visit rank is its position in the oracle's emission order for a
range that covers the whole segment of a fixture in which every entry is hit (visit_ranks: the plain ladder, a closed
query over all of T).  The order is a function of the segment's size alone -- an implicit tree over the sorted positions --
so the ranks of the umbrella ladder's entries are those of a plain ladder of as many entries (tests/test_lookup_gen_cpu.py
checks on the umbrella ladder itself that the oracle's rows come out by ascending rank of that kind).

Fixtures (unidirectional: the query sequences own no entries, so max_seg is the larger of the two ladders):
  the ladder            n disjoint records on T, record i at [20 i + 100, 20 i + 112), query side on q{i % 3}, CIGAR 12=.
                        The range (T, 20 a + 100, 20 (b - 1) + 101) has window exactly [a, b) and hits every entry of it,
                        closed test and half-open test alike.
  the umbrella ladder   the same on T2, plus one record over all of it (entry 0: every window starts there) and a
                        zero-length record (target start == end, CIGAR 5I) behind every 50th ladder record: a plain
                        window hits it (it projects to no row), a transitive one does not (first < last fails)."""
import bisect
from collections import namedtuple

WIDE_CAP, WIDE_BINS = 4096, 1024   # lookup_emit_wide_kernel's key buffer and rank bins (options wide_emit_cap / wide_emit_bins lower them)
MASK = 64                          # entries the count pass's hit mask takes, from the window's aligned start
EMIT_GRID = 4096                   # launch_lookup_emit: min(n, 4096) blocks stride over the wide list
SMALL_RANGES, SMALL_PAIRS = 64, 1 << 18  # Engine::run_small takes a plain batch of <= 64 ranges whose segments sum to <= 2^18 entries
UMBRELLA_EVERY = 50
COITREES, SORTED = 0, 1            # impg_amd.ORDER_COITREES / ORDER_SORTED

M1 = dict(transitive=True, max_depth=1, min_transitive_len=0, min_distance_between_ranges=0)
M2 = dict(transitive=True, max_depth=2, min_transitive_len=0, min_distance_between_ranges=0)


# ---- the plain model -----------------------------------------------------------------------------------------------------
def is_wide(lo, ub):
    return lo < ub and ub - (lo & ~3) > MASK


def key_domain(lo, ub, order, max_seg):
    return ub - lo if order == SORTED else max(max_seg, 1)


def bin_shift(dom, bins=WIDE_BINS):
    """The smallest shift with (dom - 1) >> shift < bins: every key below dom in a bin below `bins`."""
    shift = 0
    while (dom - 1) >> shift >= bins:
        shift += 1
    return shift


def kernel_shift(dom, bins=WIDE_BINS):
    """The same number the way lookup_emit_wide_kernel computes it (the rule the shift-edge cases are about)."""
    shift = 0
    while (dom >> shift) > bins:
        shift += 1
    if dom >> shift == bins and dom & ((1 << shift) - 1):
        shift += 1
    return shift


Plan = namedtuple("Plan", "path passes shift groups")  # path: lane | single | grouped | overflow; groups: hits per group


def emit_plan(lo, ub, ranks, order, max_seg, cap=WIDE_CAP, bins=WIDE_BINS):
    """ranks: the visit rank of every hit of the window (ORDER_SORTED: its place in the window)."""
    if not is_wide(lo, ub):
        return Plan("lane", 0, 0, ())
    shift = bin_shift(key_domain(lo, ub, order, max_seg), bins)
    if len(ranks) <= cap:
        return Plan("single", 0, shift, (len(ranks),))
    hist = [0] * bins
    for r in ranks:
        hist[r >> shift] += 1
    if max(hist) > cap:
        return Plan("overflow", 0, shift, ())
    groups, acc = [], 0
    for c in hist:  # the greedy cut: a bin that would take the group past cap opens the next one
        if acc + c > cap:
            groups.append(acc)
            acc = 0
        acc += c
    groups.append(acc)
    return Plan("grouped", len(groups), shift, tuple(groups))


COUNTERS = ("lookup_wide_windows", "lookup_wide_single", "lookup_wide_grouped", "lookup_wide_group_passes", "lookup_wide_overflow")


def counters_of(plans):
    """What one lookup of these windows adds to the lookup_wide_* counters."""
    n = lambda p: sum(1 for x in plans if x.path == p)
    return dict(lookup_wide_windows=n("single") + n("grouped") + n("overflow"), lookup_wide_single=n("single"),
                lookup_wide_grouped=n("grouped"), lookup_wide_group_passes=sum(x.passes for x in plans if x.path == "grouped"),
                lookup_wide_overflow=n("overflow"))


# ---- fixtures ------------------------------------------------------------------------------------------------------------
def _line(q, qlen, qs, qe, t, tlen, ts, te, cigar):
    return "%s\t%d\t%d\t%d\t+\t%s\t%d\t%d\t%d\t5\t5\t60\tcg:Z:%s" % (q, qlen, qs, qe, t, tlen, ts, te, cigar)


def ladder_len(n):
    return 20 * n + 1000


def umbrella_entries(n2):
    """The (start, end) of T2's entries in segment order: the umbrella, the ladder, the zero-length records."""
    ent = [(50, 20 * n2 + 200)]
    for i in range(n2):
        ent.append((20 * i + 100, 20 * i + 112))
        if i % UMBRELLA_EVERY == UMBRELLA_EVERY - 1:
            ent.append((20 * i + 115, 20 * i + 115))
    assert ent == sorted(ent) and len(set(s for s, _ in ent)) == len(ent)
    return ent


def ladder_entries(n):
    return [(20 * i + 100, 20 * i + 112) for i in range(n)]


def paf(n, n2=0):
    """The ladder of n records on T and, with n2, the umbrella ladder of n2 records on T2."""
    L = ladder_len(max(n, n2))
    lines = [_line("q%d" % (i % 3), L, 20 * i, 20 * i + 12, "T", L, s, e, "12=") for i, (s, e) in enumerate(ladder_entries(n))]
    if n2:
        for i, (s, e) in enumerate(umbrella_entries(n2)):
            if i == 0:
                lines.append(_line("qU", L, 0, e - s, "T2", L, s, e, "%d=" % (e - s)))
            elif s == e:
                lines.append(_line("q%d" % (i % 3), L, 20 * i, 20 * i + 5, "T2", L, s, e, "5I"))
            else:
                lines.append(_line("q%d" % (i % 3), L, 20 * i, 20 * i + 12, "T2", L, s, e, "12="))
    return "\n".join(lines) + "\n"


def ladder_range(a, b):
    """(start, end) on T whose window is [a, b), every entry of it a hit."""
    assert a < b
    return 20 * a + 100, 20 * (b - 1) + 101


def window(entries, qs, qe, transitive):
    """(lo, ub, hits) of the range [qs, qe) over a segment's (start, end) list, as lookup_count_lane_kernel defines them:
    ub = first entry with start >= qe (> for the closed test), lo = first entry whose running maximum of ends > qs (>=),
    hits = the entries of [lo, ub) whose end passes the same test -- a transitive level never hits an empty entry."""
    starts = [s for s, _ in entries]
    ub = bisect.bisect_left(starts, qe) if transitive else bisect.bisect_right(starts, qe)
    lo, run = len(entries), None
    for i, (s, e) in enumerate(entries):
        run = e if run is None else max(run, e)
        if (run > qs) if transitive else (run >= qs):
            lo = i
            break
    lo = min(lo, ub)
    hit = lambda s, e: (s < e and e > qs) if transitive else e >= qs
    return lo, ub, [i for i in range(lo, ub) if hit(*entries[i])]


def visit_ranks(c, target_id, n):
    """rank[i] of the i-th entry of an n-record ladder on `target_id` of the oracle index c: its position in the oracle's
    emission order for the closed query over the whole target (every entry a hit)."""
    rows = c.query(target_id, 0, ladder_len(n))[1:]
    assert len(rows) == n
    rank = [None] * n
    for k, t in enumerate(rows["t_first"].tolist()):
        i, rem = divmod(t - 100, 20)
        assert rem == 0 and rank[i] is None
        rank[i] = k
    return rank


def hit_ranks(lo, hits, order, rank):
    return [i - lo for i in hits] if order == SORTED else [rank[i] for i in hits]


# ---- the cases -----------------------------------------------------------------------------------------------------------
# A case: one index (n, n2, order), option settings to run under, batches of named ranges.  `limits` lists the
# (wide_emit_cap, wide_emit_bins) settings; `reach` notes what the case is there for (tests/test_lookup_gen_cpu.py checks that the
# list as a whole reaches every path and edge); forms None = all five.
Case = namedtuple("Case", "name n n2 order ranges limits modes forms reach")
PLAIN_M1_M2 = (dict(), M1, M2)


def _ladder(pairs):
    return [("T",) + ladder_range(a, b) for a, b in pairs]


def _t2_by_ub(n2, ub, back):
    """A range on T2 whose window is [0, ub) and that hits the umbrella and the last `back` entries of the window."""
    ent = umbrella_entries(n2)
    return ("T2", ent[ub - back][0], ent[ub - 1][0] + 1)


def width_boundary(n2):
    r = _ladder([(a, a + w) for a in (8, 9, 10, 11) for w in range(60, 67)])
    r += [_t2_by_ub(n2, ub, back) for ub in range(60, 68) for back in (1, 4)]
    return r


N_MAIN, N2_MAIN = 4097, 400
HIT_COUNTS = (64, 65, 255, 256, 257, 4095, 4096)


def hit_count_ranges():
    r = _ladder([(9, 9 + h) if 9 + h <= N_MAIN else (1, 1 + h) for h in HIT_COUNTS] + [(0, h) for h in HIT_COUNTS[-2:]])
    ent = umbrella_entries(N2_MAIN)
    r += [_t2_by_ub(N2_MAIN, ub, back) for ub, back in ((103, 1), (103, 2), (len(ent), 4), (260, 3))]
    r.append(("T2", ent[49][0], ent[52][0] + 1))  # entry 51 is empty: 5 hits plain (umbrella + 4), 4 transitive
    return r


def natural_group_ranges(n):
    """The full cover (n hits: groups), a window off the aligned start, and the shift edge's second range: the last 100 entries,
    one pass, among them the entry of the top rank n - 1.  On the longer ladder also windows of 4097 hits that end on the last
    entry and on entry 4096, and one of 4193."""
    pairs = [(0, n), (1, n), (n - 100, n)]
    if n > 4097:
        pairs += [(n - 4097, n), (0, 4097), (4000, n)]
    return _ladder(pairs)


def shift_edge_ranges(n):
    return _ladder([(0, n), (n - 100, n)])


SORTED_WINDOWS = (1024, 1025, 2049, 4097, 8193)


def sorted_window_ranges(n):
    return _ladder([(0, w) for w in SORTED_WINDOWS] + [(n - w, n) for w in SORTED_WINDOWS[:-1]] + [(3, 3 + 1025)])


LOWERED = ((100, 8), (64, 4), (128, 16))
N_LOW = 1000


def lowered_ranges():
    """Windows of the 1000-entry ladder swept over widths and places: under every setting of LOWERED the model must find a
    single-pass window, a grouped one of >= 3 passes and an overflow window among them (tests/test_lookup_gen_cpu.py)."""
    pairs = [(9, 9 + 64), (10, 10 + 65), (0, 100), (0, 128), (0, 129), (0, 200), (1, 256), (0, 400), (5, 700), (0, 1000), (900, 1000)]
    pairs += [(a, a + 2 * w) for a, w in ((0, 100), (300, 128))] + [(a, a + 300) for a in (0, 350, 700)]
    # (found with the model: three passes under (100, 8) -- the first three -- and under (64, 4) and (64, 8) -- the last two)
    pairs += [(280, 400), (406, 526), (665, 785), (441, 507), (700, 770)]
    return _ladder(pairs)


def many_window_ranges():
    return _ladder([(k % 330, k % 330 + 70) for k in range(5000)])


def small_batch_ranges():
    return lowered_ranges()[:9] + lowered_ranges()[-5:] + _ladder([(a, a + 70) for a in range(0, 160, 10)])


N2_FUSED = 200


def fused_t2_ranges():
    ent = umbrella_entries(N2_FUSED)
    out = []
    for k in range(200):
        ub = 66 + (k * 7) % (len(ent) - 66)
        back = 40 + (k * 11) % 50
        back = min(back, ub - 1)
        out.append(_t2_by_ub(N2_FUSED, ub, back))
    return out


BOTH = ((1, 1), (1, 0), (4096, 1), (4096, 0))  # (locality_min, fuse_final_level)
DEFAULT = ((WIDE_CAP, WIDE_BINS),)

CASES = {c.name: c for c in [
    Case("width_boundary", N_MAIN, N2_MAIN, COITREES, width_boundary(N2_MAIN), DEFAULT, PLAIN_M1_M2, None, ("lane", "single", "width_edges")),
    Case("hit_counts", N_MAIN, N2_MAIN, COITREES, hit_count_ranges(), DEFAULT, PLAIN_M1_M2, None, ("single", "hit_edges", "few_hits")),
    Case("groups_4097", 4097, 0, COITREES, natural_group_ranges(4097), DEFAULT, PLAIN_M1_M2, None, ("grouped", "shift_edge")),
    Case("groups_8193", 8193, 0, COITREES, natural_group_ranges(8193), DEFAULT, PLAIN_M1_M2, None, ("grouped", "groups_8193", "shift_edge")),
] + [
    Case("shift_coitrees_%d" % n, n, 0, COITREES, shift_edge_ranges(n), DEFAULT, (dict(), M1), None, ("shift_edge",) if n != 1024 else ("single",))
    for n in (1024, 1025, 2049)  # (4097 and 8193: natural_group_ranges holds the same two ranges, (0, n) and (n - 100, n))
] + [
    Case("shift_sorted_8193", 8193, 0, SORTED, sorted_window_ranges(8193), DEFAULT, (dict(), M1), None, ("shift_edge", "grouped")),
    Case("lowered_limits", N_LOW, 0, COITREES, lowered_ranges(), LOWERED + DEFAULT, PLAIN_M1_M2, None, ("single", "grouped3", "overflow")),
    Case("lowered_limits_sorted", N_LOW, 0, SORTED, lowered_ranges(), LOWERED + DEFAULT, (dict(), M1), None, ("single", "grouped3")),
    Case("many_windows", 400, 0, COITREES, many_window_ranges(), DEFAULT, (dict(), M1), ("stats", "attributed"), ("more_than_grid",)),
    Case("small_batch", N_LOW, 0, COITREES, small_batch_ranges(), LOWERED[:1] + DEFAULT, (dict(),), ("batch",), ("single", "overflow", "small")),
    Case("fused_t2", 0, N2_FUSED, COITREES, fused_t2_ranges(), DEFAULT, (dict(), M1), None, ("single", "empty_in_wide")),
]}


def entries_of(case, target):
    return ladder_entries(case.n) if target == "T" else umbrella_entries(case.n2)


def seg_offset(case, target):
    """Where the target's segment starts in the entry array: sequence ids follow first appearance in the PAF (q0, T, q1, q2, qU,
    T2), the query sequences own no entries."""
    return 0 if target == "T" else case.n


def max_seg(case):
    return max(case.n, len(umbrella_entries(case.n2)) if case.n2 else 0)


def plans(case, ranks, transitive, cap=WIDE_CAP, bins=WIDE_BINS):
    """The Plan and the (lo, ub, hits) -- places in the entry array -- of every range of the case.  ranks: {target name: rank list} (ORDER_COITREES; unused under ORDER_SORTED)."""
    out, memo = [], {}
    for r in case.ranges:
        if r not in memo:
            t, qs, qe = r
            lo, ub, hits = window(entries_of(case, t), qs, qe, transitive)
            off = seg_offset(case, t)
            memo[r] = emit_plan(off + lo, off + ub, hit_ranks(lo, hits, case.order, ranks.get(t)), case.order, max_seg(case), cap, bins), (off + lo, off + ub, len(hits))
        out.append(memo[r])
    return [p for p, _ in out], [w for _, w in out]
