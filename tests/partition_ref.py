"""`impg partition` restated sequentially for the tests (reference src/commands/partition.rs:158-1408, BED output).

The yardstick of test_partition_cpu.py / test_gpu_partition.py: plain Python, one row at a time, the sets kept in the
CPU restatement's SortedRanges and the queries answered by OracleIndex.query(..., masked_regions=...).  It also counts
what a run exercised, so that a test can assert its inputs reached the cases it is about."""
import bisect

import numpy as np

from oracle import oracle as o


class Sets:
    """{seq id: SortedRanges} with a cached copy of every list."""

    def __init__(self, lens, full):
        self.lens = list(lens)
        self.sr = {}
        self.cache = {}
        for s, n in enumerate(self.lens):
            self.sr[s] = o.SortedRanges(n, 0)
            self.cache[s] = []
            if full:
                self.insert(s, 0, n)

    def insert(self, s, a, b):
        self.sr[s].insert(a, b)
        self.cache[s] = None

    def get(self, s):
        if s not in self.sr:
            return None
        if self.cache[s] is None:
            self.cache[s] = self.sr[s].ranges()
        return self.cache[s]

    def reset(self, s):
        self.sr[s] = o.SortedRanges(self.lens[s], 0)
        self.cache[s] = []

    def remove(self, s):
        del self.sr[s]
        del self.cache[s]

    def table(self):
        return {s: (list(self.get(s)) if s in self.sr else []) for s in range(len(self.lens))}


def _first_relevant(ranges, p):  # binary_search_by_key + the look at the previous range (:1010-1028)
    pos = bisect.bisect_left(ranges, (p, -(1 << 62)))
    if pos < len(ranges) and ranges[pos][0] == p:
        return pos
    if pos > 0 and ranges[pos - 1][1] > p:
        return pos - 1
    return pos


def merge_overlaps(rows, d):  # :939-976 on [seq, lo, hi]
    if len(rows) <= 1 or d < 0:
        return rows
    rows = sorted(rows, key=lambda r: (r[0], r[1]))  # stable
    out = [list(rows[0])]
    for r in rows[1:]:
        c = out[-1]
        if c[0] != r[0] or r[1] > c[2] + d:
            out.append(list(r))
        else:
            c[1] = min(c[1], r[1])
            c[2] = max(c[2], r[2])
    return out


class Ref:
    def __init__(self, lens):
        self.lens = [int(x) for x in lens]
        self.masked = Sets(self.lens, full=False)
        self.missing = Sets(self.lens, full=True)
        self.count = dict(extensions=0, splits=0, empty_windows=0, boundary_extensions=0, rehomed=0)
        self.seen = set()

    def apply(self, rows, d, min_missing, min_boundary):
        """rows: (seq, q_first, q_last) triples; returns the window's [(seq, lo, hi)]."""
        norm = []
        keys = set()
        for s, a, b in rows:
            if a > b:
                self.seen.add("reverse")
            if (s, a, b) in keys:
                self.seen.add("duplicate")
            keys.add((s, a, b))
            lo, hi = min(a, b), max(a, b)
            for dist in (lo, self.lens[s] - hi):
                if dist in (199, 200, 201):
                    self.seen.add("end_dist_%d" % dist)
            norm.append([s, lo, hi])
        if not norm:  # a window the mask covers whole: the query returns nothing ("No overlaps found", :559-566)
            self.count["empty_windows"] += 1
            return []
        v = merge_overlaps(norm, d)
        if min_boundary > 0:  # :1369-1408
            for r in v:
                zero = 0
                if r[1] < min_boundary:
                    self.count["boundary_extensions"] += r[1] > 0
                    zero = r[1] > 0
                    if zero:
                        self.seen.add("boundary_to_zero")
                    r[1] = 0
                if self.lens[r[0]] - r[2] < min_boundary:
                    self.count["boundary_extensions"] += r[2] < self.lens[r[0]]
                    if r[2] < self.lens[r[0]]:
                        self.seen.add("boundary_to_len")
                    r[2] = self.lens[r[0]]
                r.append(zero)
            for s in {r[0] for r in v}:
                if sum(1 for r in v if r[0] == s and r[3]) >= 2:
                    self.seen.add("both_to_zero")
            v = [r[:3] for r in v]
        out = []
        i = 0
        while i < len(v):  # :1334-1363: runs of one sequence id
            j = i
            while j < len(v) and v[j][0] == v[i][0]:
                j += 1
            self._sequence(v[i][0], v[i:j], min_missing, out)
            i = j
        if not out:
            self.count["empty_windows"] += 1
            self.seen.add("inside_mask")
            return []
        return [tuple(r) for r in merge_overlaps(out, 0)]

    def _sequence(self, s, ivs, min_missing, out):
        miss = self.missing.get(s)
        ext = []
        if miss is not None:  # step 1
            for _, ms, me in ivs:
                for k in range(_first_relevant(miss, ms), len(miss)):
                    a, z = miss[k]
                    if a > me:
                        break
                    if a < ms < z and ms - a in (299, 300, 301):
                        self.seen.add("frag_%d" % (ms - a))
                    if a < me < z and z - me in (299, 300, 301):
                        self.seen.add("frag_%d" % (z - me))
                    if a < ms < z and 0 < ms - a < min_missing:
                        ext.append([a, ms])
                    if a < me < z and 0 < z - me < min_missing:
                        ext.append([me, z])
        self.count["extensions"] += len(ext)
        if ext:  # step 2
            ext.sort(key=lambda x: x[0])
            merged = [ext[0]]
            for x in ext[1:]:
                if x[0] <= merged[-1][1]:
                    merged[-1][1] = max(merged[-1][1], x[1])
                else:
                    merged.append(x)
            ext = merged
        masks = list(self.masked.get(s))  # as they were before this window
        buf = []
        for _, start, end in ivs:  # step 3
            for xs, xe in ext:
                if (xe >= start and xs <= start) or (xs <= end and xe >= end):
                    if xs < start and xe > end:  # one extension moves both ends: it covers the interval whole
                        self.seen.add("extension_covers_interval")
                    start = min(start, xs)
                    end = max(end, xe)
            buf.append((start, end))
            if (start, end) in masks:
                self.seen.add("equal_mask")
            if any((z == start or a == end) and a < z for a, z in masks) and not any(a < end and z > start for a, z in masks):
                self.seen.add("touching")
            cur = start
            pieces = 0
            for k in range(_first_relevant(masks, cur), len(masks)):
                a, z = masks[k]
                if a > end:
                    break
                if z <= cur:
                    continue
                if cur < a:
                    out.append([s, cur, a])
                    pieces += 1
                cur = max(cur, z)
                if cur >= end:
                    break
            if cur < end:
                out.append([s, cur, end])
                pieces += 1
            self.count["splits"] += pieces >= 2
        for a, b in buf:  # step 4
            self.masked.insert(s, a, b)
        if miss is not None:  # step 5
            masks = self.masked.get(s)
            old = list(miss)
            self.missing.reset(s)
            for a0, z0 in old:
                cur = a0
                k = _first_relevant(masks, a0)
                while k < len(masks) and cur < z0:
                    a, z = masks[k]
                    if a > z0:
                        break
                    if z <= cur:
                        k += 1
                        continue
                    if cur < a:
                        self.missing.insert(s, cur, a)
                    cur = max(cur, z)
                    k += 1
                if cur < z0:
                    self.missing.insert(s, cur, z0)
            if not self.missing.get(s):
                self.missing.remove(s)
                self.seen.add("emptied_missing")

    # ---- windows ----------------------------------------------------------------------------------------------------
    def select(self, mode, window_size, names=None):  # :715-937
        ranges = []
        present = [s for s in range(len(self.lens)) if self.missing.get(s) is not None]
        kind, _, sep = mode.partition(",")
        sep = sep or "#"
        if kind == "longest":
            best = None
            for s in present:
                for a, z in self.missing.get(s):
                    k = (z - a, s)
                    if best is None or k >= best[0]:  # max_by keeps the later of equals
                        best = (k, (s, a, z))
            if best:
                ranges.append(best[1])
        elif kind == "total":
            best = None
            for s in present:
                k = (sum(z - a for a, z in self.missing.get(s)), s)
                if best is None or k >= best[0]:
                    best = (k, s)
            if best:
                ranges.append((best[1], 0, self.lens[best[1]]))
        elif kind in ("sample", "haplotype"):
            groups = {}
            for s in present:
                f = names[s].split(sep)
                prefix = f[0] if kind == "sample" else f[0] + sep + (f[1] if len(f) > 1 else "")
                groups.setdefault(prefix, []).append(s)
            if groups:
                best = max(groups, key=lambda p: (sum(z - a for s in groups[p] for a, z in self.missing.get(s)), p))
                for s in sorted(groups[best], key=lambda s: (-self.lens[s], s)):  # ties: ascending id (documented)
                    ranges.append((s, 0, self.lens[s]))
        else:
            raise ValueError(mode)
        windows = []
        for s, start, end in ranges:
            mine = []
            pos = start
            while pos < end:
                we = min(pos + window_size, end)
                if we - pos < window_size and mine:
                    mine[-1] = (s, mine[-1][1], end)
                else:
                    mine.append((s, pos, we))
                pos = we
            windows += mine
        return windows


def starting_windows(ids, lens, window_size):  # :220-246
    windows = []
    for s in ids:
        pos, end = 0, int(lens[s])
        while pos < end:
            we = min(pos + window_size, end)
            if we - pos < window_size and windows and windows[-1][0] == s:
                windows[-1] = (s, windows[-1][1], end)
                break
            windows.append((s, pos, we))
            pos = we
    return windows


def rehome_singleton_slivers(parts):  # :45-156; returns (partitions, number of rows moved)
    if not parts:
        return parts, 0
    rows = []
    for p, (_, ivs) in enumerate(parts):
        for s, a, b in ivs:
            rows.append([s, a, b, p])
    rows.sort(key=lambda r: (r[0], r[1], r[2]))
    counts = [0] * len(parts)
    for r in rows:
        counts[r[3]] += 1
    moved = 0
    if 1 in counts:
        for _ in range(101):
            single = {p for p, c in enumerate(counts) if c == 1}
            pending = []
            for i, (c, s, e, p) in enumerate(rows):
                if p not in single:
                    continue
                left = rows[i - 1][3] if i > 0 and rows[i - 1][0] == c and rows[i - 1][2] == s else None
                right = rows[i + 1][3] if i + 1 < len(rows) and rows[i + 1][0] == c and rows[i + 1][1] == e else None
                ls = left is not None and left not in single
                rs = right is not None and right not in single
                if ls and rs:
                    t = left if counts[left] >= counts[right] else right
                elif ls:
                    t = left
                elif rs:
                    t = right
                else:
                    continue
                if t != p:
                    pending.append((i, t))
            if not pending:
                break
            for i, t in pending:
                counts[rows[i][3]] -= 1
                counts[t] += 1
                rows[i][3] = t
                moved += 1
    fresh = [[] for _ in parts]
    for s, a, b, p in rows:
        fresh[p].append((s, a, b))
    return [(parts[p][0], fresh[p]) for p in range(len(parts)) if fresh[p]], moved


def bed_text(parts, names):  # :1682-1717
    return "".join("%s\t%d\t%d\t%d\n" % (names[s], a, b, num) for num, ivs in parts for s, a, b in ivs)


def partition(index, window_size, merge_distance, min_missing_size=3000, min_boundary_distance=3000, selection_mode="longest",
              starting=None, rehome=True, max_windows=None, **query_kw):
    """partition_alignments over an OracleIndex.  Returns (Ref, partitions after rehoming, partitions.bed text)."""
    n = index.num_seqs()
    lens = [index.seq_len(s) for s in range(n)]
    names = [index.seq_name(s) for s in range(n)]
    ref = Ref(lens)
    windows = starting_windows(starting, lens, window_size) if starting else []
    if not windows:
        windows = ref.select(selection_mode, window_size, names)
    parts = []
    done = 0
    while windows:
        for s, a, b in windows:
            mask = {q: (lens[q], ref.masked.get(q)) for q in range(n)}
            res = index.query(s, a, b, masked_regions=mask, transitive=True, **query_kw)
            rows = [(int(r["query_id"]), int(r["q_first"]), int(r["q_last"])) for r in res]
            out = ref.apply(rows, merge_distance, min_missing_size, min_boundary_distance)
            if out:
                parts.append((len(parts), out))
            done += 1
        if max_windows is not None and done >= max_windows:
            break
        windows = ref.select(selection_mode, window_size, names)
    if rehome:
        parts, moved = rehome_singleton_slivers(parts)
        ref.count["rehomed"] = moved
    return ref, parts, bed_text(parts, names)


def rows_array(rows):
    """(seq, q_first, q_last) triples -> INTERVAL_DTYPE rows (the target side is not looked at)."""
    a = np.zeros(len(rows), dtype=o.INTERVAL_DTYPE)
    for i, (s, x, y) in enumerate(rows):
        a[i] = (s, x, y, 0, 0, 0)
    return a


LENS = [20000, 26000, 31000, 37000, 43000, 50000]


def scripted_windows():
    """The cases test_partition_cpu.py names, for LENS with d = 100, min_missing = 300, min_boundary = 200."""
    return [
        [(0, 5000, 6000), (0, 5000, 6000), (0, 7000, 6500)],                       # duplicate, reverse strand
        [(1, 1000, 26000 - 199), (2, 1000, 31000 - 200), (3, 1000, 37000 - 201),   # 199 / 200 / 201 from an end
         (4, 199, 500), (5, 200, 500), (3, 201, 600)],
        [(0, 7299, 8000), (0, 9000, 9500)],                                        # leaves a fragment of 299
        [(0, 9800, 10000)],                                                        # ... of 300
        [(0, 10301, 10500)],                                                       # ... of 301
        [(0, 5000, 6000)],                                                         # equal to a mask range: nothing
        [(0, 5200, 5800)],                                                         # inside the mask: nothing
        [(2, 10, 40), (2, 150, 180)],                                              # both extend to 0
        [(0, 4500, 5000)],                                                         # touches a mask range
        [(1, 0, 26000)],                                                           # empties the missing set of 1
        [(3, 500, 36000)],                                                         # split by (201, 600)'s and (1000, ...)'s masks
    ]


def random_windows(rng, lens, n_windows, max_rows=200):
    out = []
    for _ in range(n_windows):
        rows = []
        for _ in range(int(rng.integers(1, max_rows + 1))):
            s = int(rng.integers(0, len(lens)))
            ln = int(rng.integers(1, 300))
            a = int(rng.integers(0, lens[s] - ln + 1))
            r = (s, a, a + ln) if rng.random() < 0.7 else (s, a + ln, a)
            rows.append(r)
            if rng.random() < 0.05:
                rows.append(r)
        out.append(rows)
    return out


# ---- small, collision-dense universes: nesting, touching and equal coordinates in nearly every window -------------------
I32_MAX = 2 ** 31 - 1
DENSE_N_SEQ = (1, 2, 3, 4, 7, 8)
DENSE_D, DENSE_MIN_MISSING, DENSE_MIN_BOUNDARY = (0, 1, 3, 100), (0, 1, 5, 1000), (0, 1, 4, 1000)
DENSE_VARIANTS = {"plain": dict(zero_len=False, big=False), "zero_len": dict(zero_len=True, big=False),
                  "big": dict(zero_len=False, big=True)}
# what a variant's seeds together must have met (dense_reference); the zero-length variant adds ZERO_LEN_REACH
DENSE_REACH = ["fragment_extension", "extension_covers_interval", "boundary_to_zero", "boundary_to_len", "both_to_zero", "split",
               "inside_mask", "equal_mask", "touching", "emptied_everywhere"]
ZERO_LEN_REACH = "zero_length_mask_range"


def dense_case(seed, *, zero_len=False, big=False, n_windows=12):
    """(lens, (d, min_missing, min_boundary), windows): 1-8 sequences of 1-64 bases, 1-8 rows a window with both
    coordinates uniform in [0, len], parameters from 0 to beyond every length.  zero_len: rows with q_first == q_last are
    kept.  big: every length is 2^31 - 1 and every coordinate within 64 of either end."""
    rng = np.random.default_rng([int(seed), int(zero_len), int(big)])
    n_seq = int(rng.choice(DENSE_N_SEQ))
    lens = [I32_MAX] * n_seq if big else [int(x) for x in rng.integers(1, 65, n_seq)]
    params = tuple(int(rng.choice(c)) for c in (DENSE_D, DENSE_MIN_MISSING, DENSE_MIN_BOUNDARY))

    def coord(s):
        if not big:
            return int(rng.integers(0, lens[s] + 1))
        off = int(rng.integers(0, 65))
        return off if rng.random() < 0.5 else lens[s] - off

    windows = []
    for _ in range(n_windows):
        rows = []
        for _ in range(int(rng.integers(1, 9))):
            s = int(rng.integers(0, n_seq))
            a, b = coord(s), coord(s)
            while a == b and not zero_len:
                a, b = coord(s), coord(s)
            rows.append((s, a, b))
        windows.append(rows)
    return lens, params, windows


def ref_tables(ref):
    """(masked, missing) of a Ref.  A sequence of length 0 starts outside the missing map in both implementations
    (include/impg_gpu.h), where the reference keeps the range (0, 0) until a row touches it: that range is left out."""
    missing = ref.missing.table()
    for s, n in enumerate(ref.lens):
        if n == 0:
            missing[s] = []
    return ref.masked.table(), missing


def ref_steps(ref, windows, params, window_size, names=None, modes=("longest", "total")):
    """Apply the windows to `ref`; per window (rows, output rows, masked, missing, {mode: select(mode)}), for replay()."""
    steps = []
    for rows in windows:
        out = ref.apply(rows, *params)
        masked, missing = ref_tables(ref)
        steps.append((rows, params, out, masked, missing, {m: ref.select(m, window_size, names) for m in modes}))
    return steps


def replay(reg, steps, window_size, names=None):
    """A Regions object against the recorded steps of a Ref: rows, both tables and the selections after every window."""
    for k, (rows, params, out, masked, missing, sel) in enumerate(steps):
        assert reg.apply(rows_array(rows), *params) == out, (k, params, rows[:8])
        assert reg.get("masked") == masked, (k, params, rows[:8])
        assert reg.get("missing") == missing, (k, params, rows[:8])
        for mode, want in sel.items():
            assert reg.select(mode, window_size, names) == want, (k, mode, params, rows[:8])


def dense_reference(seeds, *, zero_len=False, big=False):
    """Ref over dense_case(seed) of every seed: ([(seed, lens, window size, steps)], what the seeds reached together).
    The window size is the longest length, one window a range: on 2^31 - 1 bases a small one enumerates 10^8 windows."""
    cases, reached = [], set()
    for seed in seeds:
        lens, params, windows = dense_case(seed, zero_len=zero_len, big=big)
        ref = Ref(lens)
        steps = []
        for k, rows in enumerate(windows):
            if all(ref.missing.get(s) is None for s in range(len(lens))):
                reached.add("emptied_everywhere")  # every missing set has emptied, and a further window is applied
            steps += ref_steps(ref, [rows], params, max(lens))
            if any(a == z for v in steps[-1][3].values() for a, z in v):
                reached.add(ZERO_LEN_REACH)
        reached |= ref.seen
        reached |= {name for name, key in (("fragment_extension", "extensions"), ("split", "splits")) if ref.count[key]}
        cases.append((seed, lens, max(lens), steps))
    return cases, reached


def sparse_case(n_seq):
    """Many sequences, few of them touched, a few of length 0 (rows on those are (s, 0, 0))."""
    rng = np.random.default_rng([77, n_seq])
    lens = [int(x) for x in rng.integers(1, 400, n_seq)]
    for s in range(3, n_seq, 61):
        lens[s] = 0
    hot = sorted({0, n_seq // 2, n_seq - 1, min(3, n_seq - 1)} | {int(x) for x in rng.integers(0, n_seq, 3)})
    windows = []
    for _ in range(6):
        rows = []
        for _ in range(int(rng.integers(1, 7))):
            s = hot[int(rng.integers(0, len(hot)))]
            a, b = (int(x) for x in rng.integers(0, lens[s] + 1, 2))
            if a != b or lens[s] == 0:
                rows.append((s, a, b))
        windows.append(rows or [(0, 0, lens[0])])
    return lens, (1, 5, 4), windows


def row_count_case(n):
    """n rows that stay n intervals (d = 0, gaps of 3), in random order and strand on two sequences: a fresh mask
    (n_old = 0), n intervals each split by the warm one, 2n fragment extensions, then n intervals swallowed whole.
    [(rows, params)] per window."""
    rng = np.random.default_rng([78, n])
    lens = [8 * ((n + 1) // 2) + 20] * 2

    def rows(a, b):
        out = [(i % 2, 8 * (i // 2) + a, 8 * (i // 2) + b) for i in range(n)]
        out = [r if rng.random() < 0.7 else (r[0], r[2], r[1]) for r in out]
        return [out[i] for i in rng.permutation(n)]

    first = rows(1, 3)
    return lens, [(first, (0, 0, 0)), (rows(2, 5), (0, 0, 0)), (rows(7, 8), (0, 3, 0)), (first, (0, 0, 0))]


def piece_count_case():
    """Windows whose subtraction of the old mask leaves exactly the stated number of pieces (none of them touch, so the
    window's output has as many rows): (lens, params, [(rows, pieces)])."""
    return [100, 100], (0, 0, 0), [([(0, 10, 20), (0, 30, 40)], 2), ([(0, 12, 18)], 0), ([(0, 15, 25)], 1), ([(0, 5, 28)], 2),
                                   ([(0, 30, 40)], 0), ([(1, 7, 9)], 1), ([(0, 0, 50), (1, 0, 9)], 4)]


def clamp_case():
    """(lengths as given, lengths as both implementations keep them, params, windows at the clamped end; the last has
    a zero-length row at 2^31 - 1 itself behind a mask range of its sequence)."""
    e = I32_MAX
    return [2 ** 33, 100], [e, 100], (0, 5, 4), [[(0, e - 10, e - 6)], [(0, e - 30, e - 20), (0, e - 3, e)], [(0, e - 50, e - 40), (0, e, e)],
                                                [(0, e, e - 100)]]


TIE_NAMES = ["S%d#%d#c%d" % (k % 5, k % 3, k) for k in range(40)]


def tie_case():
    """40 sequences of 1000 bases, every row a whole hundred: the missing ranges, the sequences' sums and the groups'
    sums tie all the time."""
    rng = np.random.default_rng(79)
    windows = []
    for _ in range(12):
        windows.append([(int(s), 100 * int(j), 100 * int(j) + 100) for s, j in zip(rng.integers(0, 40, 10), rng.integers(0, 10, 10))])
    return [1000] * 40, (0, 0, 0), windows


REFUSAL_NAMES = ["A#1#c", "B#1#c", "B#2#c"]


def refusal_case(fresh):
    """(lens, params, windows applied first, valid rows of the refused call, a window for afterwards).  The valid rows
    alone would move the winner of `total`, `sample` and `haplotype` to another sequence or group."""
    lens = [1000, 900, 800]
    if fresh:  # sums 1000 / 900 / 800; the valid rows alone: 50 / 900 / 800
        return lens, (0, 0, 0), [], [(0, 0, 950)], [(1, 100, 300)]
    # sums 500 / 800 / 800; the valid rows alone: 500 / 100 / 100
    return lens, (0, 0, 0), [[(0, 0, 500)], [(1, 100, 200)]], [(1, 200, 900), (2, 0, 700)], [(2, 100, 300)]
