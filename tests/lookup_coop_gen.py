"""Inputs that send the waves of the cooperative count kernel (kernels.hip: lookup_count_coop_kernel) down a chosen path, and a
plain model that says which of its three paths every wave of a batch takes.

The kernel runs when a level has a lookup order (option locality_min 1 forces one).  The model restates, from the fixture
and the batch alone:
  order_key    where a range's window is expected in the entry array: segment start + floor(start * n / sequence length),
               capped at the segment's last entry; 0 for an unknown target.  The level's ranges are sorted by it, stably;
  waves        the sorted ranges in groups of 64; the last group may be short;
  path         "mixed"  the wave's ranges name more than one target, an unknown one, or one without entries;
               "span"   else, with L2 = l2(min start), L1a = l1(min end), L1b = l1(max end) over the segment (the lane
                        kernel's two boundary searches, lookup_gen.window), S0 = (a + min(L2, L1a)) & ~3 and S1 = a + L1b in
                        places of the entry array: S1 - S0 > lookup_coop_span;
               "coop"   else.
It is used only to say what an input reaches (the lookup_coop_waves / lookup_lane_waves_* counters of
tests/test_gpu_lookup_coop.py) -- never as the expected output of a query: that is the oracle's.

Fixtures are unidirectional PAFs of named targets with listed (start, end) entries, starts distinct, so that a segment's order
is the list's; every record's query side lies on q0 / q1 / q2, which own no entries: targets with an empty segment.  Sequence
ids follow first appearance in the text (query name, then target name), segments lie unpadded in sequence-id order.

A window with l1 < l2 (lo = ub = l1) cannot be built from records: pmax[l1] >= end[l1] >= start[l1] >= range end > range
start, so the running maximum at l1 always passes and l2 <= l1.  Only a range with start >= end could get there, and the
engine refuses those before any lookup (check_ranges, IMPG_E_INVALID; a frontier record of a deeper level is a projected
interval, first < last).  The empty windows here are the ones with l2 = l1: ranges in a gap between entries, before the first
entry and behind the last end.

The wave's searches take one of three shapes by the segment's size n (search_shape): "block" n <= 64, no sampled level: one
round over the entries; "samples" up to 256 samples (n <= 16 384): the samples in one counting round, then the block;
"narrow" more samples: coop_narrow first cuts each search's range of samples 64 probes a round (step = ceil(width / 64), the
probes clamped to the last sample, "no probe passes" ends with the answer n) until at most 256 remain.  narrow_trace replays
that loop for one threshold."""
from collections import namedtuple

from tests import lookup_gen as lg

CAP = 256          # LOOKUP_COOP_CAP: entries a wave stages at most (option lookup_coop_span lowers it)
WAVE = 64
BAD = "#unknown"   # a range on a sequence id the index does not have
COUNTERS = ("lookup_coop_waves", "lookup_lane_waves_mixed", "lookup_lane_waves_span")
M1 = lg.M1

Fixture = namedtuple("Fixture", "name targets")  # targets: ((name, sequence length, ((start, end), ...)), ...)
Layout = namedtuple("Layout", "ids n_seq seg")   # ids: {name: sequence id}; seg: {name: (a, n, length, entries)}


# ---- fixtures ------------------------------------------------------------------------------------------------------------
def paf(fx):
    qlen = max(L for _, L, _ in fx.targets)
    lines = []
    for name, L, ent in fx.targets:
        assert list(ent) == sorted(ent) and len({s for s, _ in ent}) == len(ent) and all(0 <= s <= e <= L for s, e in ent), name
        for i, (s, e) in enumerate(ent):
            span = e - s
            lines.append("q%d\t%d\t0\t%d\t+\t%s\t%d\t%d\t%d\t5\t5\t60\tcg:Z:%s" % (i % 3, qlen, span or 5, name, L, s, e, "%d=" % span if span else "5I"))
    return "\n".join(lines) + "\n"


def layout(fx):
    ids = {}
    for name, _, ent in fx.targets:
        for i in range(min(len(ent), 3)):
            ids.setdefault("q%d" % i, len(ids))
            ids.setdefault(name, len(ids))
    own = {name: (L, ent) for name, L, ent in fx.targets}
    seg, a = {}, 0
    for name in sorted(ids, key=ids.get):
        L, ent = own.get(name, (max(L for _, L, _ in fx.targets), ()))
        seg[name] = (a, len(ent), L, tuple(ent))
        a += len(ent)
    return Layout(ids, len(ids), seg)


def ladder(n):
    return tuple(lg.ladder_entries(n))


def r_entries():
    """100 entries 1000 apart from 5000 on, 300 long -- but every tenth (j % 10 == 3) 4500 long: the running maximum of ends stays
    at its end over the next four entries -- and every tenth (j % 10 == 7) of length zero: INT_MIN in ends_t."""
    out = []
    for j in range(100):
        s = 1000 * j + 5000
        out.append((s, s + (4500 if j % 10 == 3 else 0 if j % 10 == 7 else 300)))
    return tuple(out)


SIZES = (1, 63, 64, 65, 127, 128, 4095, 4096, 4097)
# ... and the edges of this kernel's own search shapes: 256 samples (the last size searched in one counting round), 257 (the
# first narrowed: 16 385 entries, and 16 448 with a whole last block), 313 (step 5, the upper probes clamped to the last sample)
NARROW_SIZES = (16383, 16384, 16385, 16448, 20000)
FX_AB = Fixture("ab", (("A", lg.ladder_len(300), ladder(300)), ("B", lg.ladder_len(200), ladder(200))))
FX_SIZES = Fixture("sizes", tuple(("S%d" % n, lg.ladder_len(n), ladder(n)) for n in SIZES))
FX_NARROW = Fixture("narrow", tuple(("N%d" % n, lg.ladder_len(n), ladder(n)) for n in NARROW_SIZES))
FX_R = Fixture("r", (("P", 1000, ladder(5)), ("R", 200000, r_entries())))  # (P's five entries put R's segment off the vector boundary)


# ---- the plain model -----------------------------------------------------------------------------------------------------
def order_key(lay, target, start):
    if target == BAD:
        return 0
    a, n, L, _ = lay.seg[target]
    rel = max(start, 0) * n // L if L > 0 else 0
    return a + min(rel, n - 1 if n else 0)


def lookup_order(lay, ranges):
    keys = [order_key(lay, t, s) for t, s, _ in ranges]
    return sorted(range(len(ranges)), key=lambda i: keys[i])  # (stable)


def l1(entries, qe, transitive):
    """first entry with start >= qe (> for the closed test), else their number"""
    for i, (s, _) in enumerate(entries):
        if (s >= qe) if transitive else (s > qe):
            return i
    return len(entries)


def l2(entries, qs, transitive):
    """first entry whose running maximum of ends > qs (>=), else their number"""
    run = None
    for i, (_, e) in enumerate(entries):
        run = e if run is None else max(run, e)
        if (run > qs) if transitive else (run >= qs):
            return i
    return len(entries)


def search_shape(n):
    """how the wave searches a segment of n entries: block | samples | narrow"""
    return "block" if n <= 64 else "samples" if (n + 63) // 64 <= 256 else "narrow"


def narrow_trace(n, first):
    """coop_narrow over the samples of a segment of n entries for a threshold whose first passing ENTRY is `first` (n: none):
    the rounds as (step, probes clamped to the last sample, index of the first passing probe or None)."""
    cnt = (n + 63) // 64
    passes = lambda j: min(n, 64 * (j + 1)) - 1 >= first  # sample j = the last entry of block j
    l, h, out = 0, cnt, []
    while h - l > 256:
        step = (h - l + 63) // 64
        idx = [min(l + (k + 1) * step - 1, h - 1) for k in range(64)]
        clamped = sum(1 for k in range(64) if l + (k + 1) * step - 1 > h - 1)
        k = next((k for k in range(64) if passes(idx[k])), None)
        out.append((step, clamped, k))
        if k is None:
            l = h
            break
        h, l = idx[k], l + k * step
    return out


def wave_path(lay, wave, transitive, span=CAP):
    """wave: the ranges of one wave.  -> (path, S0, S1) -- places in the entry array (0, 0 for a mixed wave)"""
    targets = {t for t, _, _ in wave}
    t = next(iter(targets))
    if len(targets) != 1 or t == BAD or lay.seg[t][1] == 0:
        return "mixed", 0, 0
    a, _, _, ent = lay.seg[t]
    L2 = l2(ent, min(s for _, s, _ in wave), transitive)
    L1a = l1(ent, min(e for _, _, e in wave), transitive)
    L1b = l1(ent, max(e for _, _, e in wave), transitive)
    S0, S1 = (a + min(L2, L1a)) & ~3, a + L1b
    return ("span" if S1 - S0 > span else "coop"), S0, S1


def wave_paths(lay, ranges, transitive, span=CAP):
    """The path of every wave of one lookup of `ranges`, in wave order, and the waves (lists of range indices)."""
    order = lookup_order(lay, ranges)
    waves = [order[k:k + WAVE] for k in range(0, len(order), WAVE)]
    return [wave_path(lay, [ranges[i] for i in w], transitive, span)[0] for w in waves], waves


def windows(lay, ranges, transitive):
    """(lo, ub, hits) of every range in places of the entry array (an unknown target: no window)"""
    out = []
    for t, qs, qe in ranges:
        if t == BAD:
            out.append((0, 0, 0))
            continue
        a, _, _, ent = lay.seg[t]
        lo, ub, hits = lg.window(list(ent), qs, qe, transitive)
        out.append((a + lo, a + ub, len(hits)))
    return out


def counters_of(lay, ranges, transitive, span=CAP, coop=True):
    """What one lookup of these ranges under a lookup order adds to the three wave counters and to the lookup_wide_* ones."""
    paths, _ = wave_paths(lay, ranges, transitive, span)
    n = lambda p: sum(1 for x in paths if x == p) if coop else 0
    win = windows(lay, ranges, transitive)
    assert all(h <= lg.WIDE_CAP for _, _, h in win)  # (every wide window here is sorted in one pass)
    wide = sum(1 for lo, ub, _ in win if lg.is_wide(lo, ub))
    return dict(lookup_coop_waves=n("coop"), lookup_lane_waves_mixed=n("mixed"), lookup_lane_waves_span=n("span"),
                lookup_wide_windows=wide, lookup_wide_single=wide, lookup_wide_grouped=0, lookup_wide_group_passes=0, lookup_wide_overflow=0)


# ---- the cases -----------------------------------------------------------------------------------------------------------
# A case: one fixture, batches of ranges (each batch one lookup), the lookup_coop_span settings to run under.
Case = namedtuple("Case", "name fixture batches spans")
BATCH_SIZES = (1, 63, 64, 65, 255, 256, 257, 320)


def _lad(target, a, b):
    return (target,) + lg.ladder_range(a, b)


def batch_size_batches():
    return [[_lad("A", 3 * k % 250, 3 * k % 250 + 1 + k % 5) for k in range(n)] for n in BATCH_SIZES]


def _near(target, p, n):
    return [_lad(target, p + k % 3, p + k % 3 + 1 + k % 2) for k in range(n)]


def target_boundary_batches():
    q0 = [("q0", 100 + k, 200 + k) for k in range(64)]
    return [
        _near("A", 40, 1) + _near("B", 40, 63),    # the target changes after lane 0
        _near("A", 40, 32) + _near("B", 40, 32),   # ... after lane 31
        _near("A", 40, 63) + _near("B", 40, 1),    # ... before lane 63
        _near("A", 40, 63) + [(BAD, 10, 20)],      # an unknown target (key 0: lane 0) in an otherwise uniform wave
        _near("A", 40, 31) + [(BAD, 10, 20)] + _near("A", 40, 32),
        q0,                                        # one target, no entries
        q0[:1] + _near("A", 40, 63),
        _near("A", 40, 64) + _near("B", 40, 64),   # the boundary between two waves: both cooperative
    ]


def segment_size_batches():
    out = []
    for n in SIZES:
        centres = sorted({0, min(62, n - 1), n - 1} | ({n // 2} if n > 200 else set()))
        b = []
        for c in centres:
            p = max(0, min(c - 1, n - 4))
            b += [_lad("S%d" % n, min(p + k % 3, n - 1), min(p + k % 3 + 1 + k % 2, n)) for k in range(64)]
        out.append(b)
    return out


def narrow_batches():
    """per size: 64 ranges each at the first, a middle and the last block, and 64 behind the last end (no probe passes)"""
    out = []
    for n in NARROW_SIZES:
        t, b = "N%d" % n, []
        for c in (0, n // 2, n - 3):
            b += [_lad(t, c + k % 2, c + k % 2 + 1 + k % 2) for k in range(64)]
        last_end = lg.ladder_entries(n)[-1][1]
        b += [(t, last_end + 5 + k, last_end + 50 + k) for k in range(64)]
        out.append(b)
    return out


SPANS = (8, 64, CAP)
SPAN_WIDTHS = (8, 9, 64, 65, CAP, CAP + 1)


def span_batches():
    """one wave each: 63 windows [p, p + 1) and one [p, p + w), p on a vector boundary: the wave's span is w"""
    return [[_lad("A", 4, 5)] * 40 + [_lad("A", 4, 4 + w)] + [_lad("A", 4, 5)] * 23 for w in SPAN_WIDTHS]


def reduction_batches():
    # one key (starts 20100 .. 20163 of R: floor(start / 2000) = 10), starts descending by lane: the minimum start in lane 63; the
    # lengths put the smallest end into lane 20 and the largest -- behind the whole segment -- into lane 40
    lens = [100 + 397 * k % 30000 for k in range(64)]
    lens[20], lens[40] = 1, 170000
    return [[("R", 20163 - k, 20163 - k + lens[k]) for k in range(64)]]


def position_batches():
    ent = r_entries()
    b = [("R", 0, 100), ("R", 0, 5001), ("R", 10, 4999), ("R", 0, 5000), ("R", 150000, 150100), ("R", 104300, 104400), ("R", 199000, 200000)]
    for j in range(0, 100, 3):
        s, e = ent[j]
        b += [("R", s + 400, s + 900), ("R", s + 10, s + 20), ("R", s - 100, s + 100)]  # a gap (unless a long entry covers it), inside, across the start
    return [b, b[:64]]


def edge_batches():
    ent = r_entries()
    b = []
    for j in range(1, 100, 2):
        s, e = ent[j]
        b += [("R", s - 50, s), ("R", s - 50, s + 1), ("R", s - 50, s - 1)]          # range end = / behind / before an entry's start
        b += [("R", max(e, s + 1), max(e, s + 1) + 50), ("R", max(e, s + 1) - 1, max(e, s + 1) + 50)]  # range start = / before a running maximum
        b += [("R", s - 10, s + 10)]                                                 # across an entry (j % 10 == 7: one of length zero)
    return [b]


def wide_batches():
    """windows of 64 and of 65 entries counted from the aligned start, among narrow ones: A's segment starts at place 0"""
    w = [_lad("A", 8, 72), _lad("A", 8, 73), _lad("A", 9, 72), _lad("A", 9, 73), _lad("A", 11, 75), _lad("A", 11, 76)]
    return [_near("A", 8, 30) + w + _near("A", 8, 28)]


CASES = {c.name: c for c in [
    Case("batch_sizes", FX_AB, batch_size_batches(), (CAP,)),
    Case("target_boundary", FX_AB, target_boundary_batches(), (CAP,)),
    Case("segment_sizes", FX_SIZES, segment_size_batches(), (CAP,)),
    Case("narrowing", FX_NARROW, narrow_batches(), (CAP,)),
    Case("span_limit", FX_AB, span_batches(), SPANS),
    Case("reductions", FX_R, reduction_batches(), (CAP,)),
    Case("window_positions", FX_R, position_batches(), (CAP,)),
    Case("comparison_edges", FX_R, edge_batches(), (CAP,)),
    Case("wide_rule", FX_AB, wide_batches(), (CAP,)),
]}
