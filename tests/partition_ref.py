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
                    r[1] = 0
                if self.lens[r[0]] - r[2] < min_boundary:
                    self.count["boundary_extensions"] += r[2] < self.lens[r[0]]
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
