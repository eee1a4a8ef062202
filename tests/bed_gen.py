"""Inputs and plain statements for the tests of the device BED merge and text (impg_amd/csrc/bed_device.hip):
collision-dense row sets, the text a merged row prints, and the number of pieces the text stream cuts it into.
Inputs and arithmetic only; the merges themselves are checked against the oracle, not restated here."""
import itertools

import numpy as np

import impg_amd

# (merge distance, merge_strands): every call of the dense tests
DISTANCES = (-1, 0, 1, 2, 5)
MODES = [(d, ms) for d in DISTANCES for ms in (True, False)]
# the grid of the dense sets: coordinate universe, longest row, sequence ids per axis, zero-length rows, starts below zero
DENSE_GRID = list(itertools.product((6, 12, 40), (1, 3, 8), (1, 2), (False, True), (False, True)))
SETS_PER_CELL = 84  # 72 cells: 6 048 sets of 0 .. 13 rows, at most 78 624 rows
MAX_ROWS = 13

# the pair on which `next_start > curr_end + merge_distance` (main.rs:12523) differs between an i32 sum that wraps, as the
# reference's release build computes it, and a wider sum: 2000000100 + 147483548 = 2^31 wraps below zero, so the second
# row starts a run of its own; one less and the sum is 2^31 - 1 >= 2000000500, one run
OVERFLOW_PAIR = [(0, 2000000000, 2000000100, 0, 0, 100), (0, 2000000500, 2000000600, 1, 0, 100)]
OVERFLOW_CASES = ((147483548, 2), (147483547, 1))  # (merge distance, rows out)


def intervals(rows):
    """[(query_id, q_first, q_last, target_id, t_first, t_last)] -> INTERVAL_DTYPE"""
    a = np.zeros(len(rows), dtype=impg_amd.INTERVAL_DTYPE)
    for i, r in enumerate(rows):
        a[i] = tuple(r)
    return a


def dense_set(rng, universe, max_len, n_ids, zero_len, below_zero):
    """One small row set: few coordinates, short rows, so equal starts, contained rows, rows that meet through a third
    and cross-strand ties are the rule."""
    n = int(rng.integers(0, MAX_ROWS + 1))
    iv = np.zeros(n, dtype=impg_amd.INTERVAL_DTYPE)
    start = rng.integers(-3 if below_zero else 0, universe, n)
    ln = rng.integers(0 if zero_len else 1, max_len + 1, n)
    rev = rng.random(n) < 0.4
    iv["q_first"] = np.where(rev, start + ln, start)  # (a zero-length row is a forward one: first <= last)
    iv["q_last"] = np.where(rev, start, start + ln)
    iv["query_id"] = rng.integers(0, n_ids, n)
    iv["target_id"] = rng.integers(0, n_ids, n)
    t = rng.integers(0, universe, n)
    iv["t_first"] = t
    iv["t_last"] = t + rng.integers(1, max_len + 1, n)
    return iv


def dense_sets(seed=20261019):
    """The dense sets, cell by cell of DENSE_GRID; the same list on every call."""
    rng = np.random.default_rng(seed)
    return [dense_set(rng, *cell) for cell in DENSE_GRID for _ in range(SETS_PER_CELL)]


def batch(sets, order=None, interleave=False):
    """Row sets -> (rows, row_range) of one call, set k as range order[k] (default: k).  interleave: the rows of the
    ranges dealt round-robin into the array instead of range after range; a range's own rows keep their order."""
    order = list(range(len(sets))) if order is None else list(order)
    rows = np.concatenate(sets) if sets else np.zeros(0, dtype=impg_amd.INTERVAL_DTYPE)
    rr = np.concatenate([np.full(len(s), order[k], dtype=np.uint32) for k, s in enumerate(sets)]) if sets else np.zeros(0, dtype=np.uint32)
    if interleave:
        rank = np.concatenate([np.arange(len(s)) for s in sets])  # position inside the own range
        perm = np.lexsort((rr, rank))  # by position, then by range: stable inside a range
        rows, rr = rows[perm], rr[perm]
    return rows, rr


def merged_tuple(x):
    """an interval the oracle's merge returned -> (query id, start, end, strand) as the device reports a merged row"""
    a, b = int(x["q_first"]), int(x["q_last"])
    return (int(x["query_id"]), min(a, b), max(a, b), 0 if a <= b else 1)


def subsequence_origin(name):
    """"base:START-END" (main.rs:4642-4678) -> (base, START), else None: the text behind the last ':' up to its first '-'
    is an optional '+' and at least one digit, the number at most 2^31 - 1."""
    colon = name.rfind(":")
    if colon < 0:
        return None
    dash = name.find("-", colon + 1)
    if dash < 0:
        return None
    num = name[colon + 1:dash]
    if num.startswith("+"):
        num = num[1:]
    if not num or any(ch not in "0123456789" for ch in num) or int(num) > 2 ** 31 - 1:
        return None
    return name[:colon], int(num)


def expected_line(query_id, start, end, strand, range_name, names, original):
    """The text of one merged row: name \\t (start + shift) mod 2^32 \\t (end + shift) mod 2^32 \\t range name \\t . \\t
    strand \\n.  names: the handle's sequence names; an id beyond them prints as a decimal with no shift."""
    name, shift = str(query_id), 0
    if query_id < len(names):
        name = names[query_id]
        o = subsequence_origin(name) if original else None
        if o:
            name, shift = o
    return ("%s\t%d\t%d\t%s\t.\t%s\n" % (name, (start + shift) % 2 ** 32, (end + shift) % 2 ** 32, range_name, "+-"[strand])).encode()


def piece_count(lengths, piece):
    """Pieces the text stream sends for rows of these byte lengths: a piece takes rows [r0, r1), r1 the largest index
    whose offset is at most `piece` beyond r0's, and at least one row."""
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    r0, pieces = 0, 0
    while r0 < len(lengths):
        r1 = r0 + 1
        while r1 < len(lengths) and off[r1 + 1] - off[r0] <= piece:
            r1 += 1
        r0 = r1
        pieces += 1
    return pieces
