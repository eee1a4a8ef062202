"""`impg refine` restated sequentially for the tests (reference src/commands/refine.rs:144-876, text of
src/main.rs:7817-7861).

The yardstick of test_refine_cpu.py / test_gpu_refine.py: plain Python, one row at a time, the queries answered by
OracleIndex.query (rows in emission order) and max_entities counted over OracleIndex.target_entries.  Two things are
restated rather than copied, as include/impg_gpu.h documents them: the early break out of the hash-map walk (:758-763)
is the clamp of the count with every survivor kept, and a name without the separator has no PanSN key (what sweepga's
extract_pansn_key returns for it is unpinned)."""
import math

HOLE = 0xFFFFFFFF
NO_KEY = 0xFFFFFFFF  # entity_of[]: the sequence has no key
I32_MAX = (1 << 31) - 1


def pansn_key(name, level, sep="#"):
    """Level 'sequence': the name; 'sample': the first field; 'haplotype': the first two.  None: no key."""
    if level == "sequence":
        return name
    parts = name.split(sep)
    if len(parts) < 2:
        return None
    return parts[0] if level == "sample" else sep.join(parts[:2])


def should_merge(a, b, d):  # :834-850 on [qs, qe, ts, te]
    if d < 0:
        return False
    query_adjacent = min(abs(a[1] - b[0]), abs(a[0] - b[1])) <= d
    target_adjacent = min(abs(a[3] - b[2]), abs(a[2] - b[3])) <= d
    return query_adjacent or target_adjacent


def merge_intervals(intervals, d):  # :799-832
    if not intervals:
        return intervals
    if d < 0:
        return intervals
    intervals = sorted(intervals, key=lambda v: (v[0], v[1]))  # sort_by is stable, and so is sorted()
    merged = []
    current = list(intervals[0])
    for nxt in intervals[1:]:
        if should_merge(current, nxt, d):
            current[0] = min(current[0], nxt[0])
            current[1] = max(current[1], nxt[1])
            current[2] = min(current[2], nxt[2])
            current[3] = max(current[3], nxt[3])
        else:
            merged.append(current)
            current = list(nxt)
    merged.append(current)
    return merged


def covers_boundaries(t_start, t_end, region_start, region_end, left_threshold, right_threshold):  # :785-797
    return t_start <= region_start and t_end >= region_end and t_end >= left_threshold and t_start <= right_threshold


def blacklisted(ranges, q_lo, q_hi):
    """coitrees query(first, last) over intervals stored first = start, last = end (:736-748; the overlap rule of the
    oracle's COITree): both ends inclusive on both sides."""
    return any(a <= q_hi and b >= q_lo for a, b in ranges)


def support(rows, target_id, region_start, region_end, span_bp, merge_distance, key_of=None, max_entities=None, blacklist=None):
    """compute_support_sets (:665-783) on rows [(query_id, q_first, q_last, target_id, t_first, t_last)] in emission
    order.  key_of(seq id) -> key or None (None: identity); blacklist {seq id: [(start, end)]}.  Returns (count,
    [(seq id, q_lo, q_hi)] in ascending seq id).  A row with query_id HOLE is no row."""
    rows = [r for r in rows if r[0] != HOLE]
    if len(rows) <= 1:  # :680-682
        return 0, []
    per_sample = {}
    for r in rows:
        if r[0] == target_id:  # :687-689
            continue
        per_sample.setdefault(r[0], []).append([min(r[1], r[2]), max(r[1], r[2]), min(r[4], r[5]), max(r[4], r[5])])
    effective_span = min(max(region_end - region_start, 0), max(span_bp, 0))  # :707
    left_threshold = region_start + effective_span
    right_threshold = region_end - effective_span
    aggregated = set()
    survivors = []
    for sample_id in sorted(per_sample):
        merged = merge_intervals(per_sample[sample_id], merge_distance)
        query_range = None
        for m in merged:
            if covers_boundaries(m[2], m[3], region_start, region_end, left_threshold, right_threshold):
                q_start, q_end = min(m[0], m[1]), max(m[0], m[1])
                query_range = (q_start, q_end) if query_range is None else (min(query_range[0], q_start), max(query_range[1], q_end))
        if query_range is None:
            continue
        if blacklist is not None and blacklisted(blacklist.get(sample_id, ()), query_range[0], query_range[1]):
            continue
        survivors.append((sample_id, query_range[0], query_range[1]))  # :750-755, before the key is looked up
        key = sample_id if key_of is None else key_of(sample_id)
        if key is not None:
            aggregated.add(key)
    count = len(aggregated)
    if max_entities is not None:
        count = min(count, max_entities)  # the deterministic content of :758-763
    return count, survivors


def max_extension_bp(max_extension, locus_len):  # :177-185
    v = math.ceil(locus_len * max_extension) if max_extension <= 1.0 else math.ceil(max_extension)
    return max(min(max(v, 0), I32_MAX), 0)


def build_flanks(max_extension, step):  # :852-876
    flanks = []
    current = 0
    if max_extension == 0:
        return [0]
    while current <= max_extension:
        flanks.append(current)
        if max_extension - current < step:
            break
        current = min(current + step, I32_MAX)  # saturating_add
    if flanks[-1] != max_extension:
        flanks.append(max_extension)
    return sorted(set(flanks))


def compare_greater(a, b):
    """compare_candidates(a, b) == Greater (:564-582) on dicts with start, end, left, right, count."""
    ka = (a["count"], -(a["left"] + a["right"]), -max(a["left"], a["right"]), -(a["end"] - a["start"]))
    kb = (b["count"], -(b["left"] + b["right"]), -max(b["left"], b["right"]), -(b["end"] - b["start"]))
    return ka > kb


def update_best(best, cand):  # :548-562
    if best is None:
        return cand
    return cand if compare_greater(cand, best) else best


class Refine:
    """run_refine over an OracleIndex.  level: 'sequence' | 'sample' | 'haplotype'; query_kw: the keywords of
    oracle.make_params (transitive, dfs, max_depth, multi_impg, ...); subset_keep: per sequence id or None; blacklist:
    {seq id: [(start, end)]}."""

    def __init__(self, oracle, span_bp=1000, max_extension=0.5, extension_step=1000, merge_distance=0, level="sequence", separator="#",
                 subset_keep=None, blacklist=None, query_kw=None):
        self.c = oracle
        self.span_bp, self.max_extension, self.extension_step, self.merge_distance = span_bp, max_extension, extension_step, merge_distance
        self.level, self.sep, self.subset_keep, self.blacklist = level, separator, subset_keep, blacklist
        self.query_kw = dict(query_kw or {})
        try:
            self.names = [oracle.seq_name(i) for i in range(oracle.num_seqs())]
        except AttributeError:  # an index made without names (tracepoint arrays)
            self.names = ["seq%d" % i for i in range(oracle.num_seqs())]
        self.seen = set()  # what the runs exercised
        self.evaluations = 0

    def key_of(self, seq):
        return pansn_key(self.names[seq], self.level, self.sep)

    def compute_max_entities(self, target_id):  # :589-632
        target_key = self.key_of(target_id)
        keys = set()
        for first, last, qid, flags in self.c.target_entries(target_id):
            qid = int(qid)
            if qid == target_id:
                continue
            if self.subset_keep is not None and not self.subset_keep[qid]:
                continue
            key = self.key_of(qid)
            if key is not None and key != target_key:
                keys.add(key)
        return len(keys)

    def evaluate(self, target_id, orig_start, orig_end, seq_len, left, right, max_entities):  # :412-479
        start = max(orig_start - left, 0)
        end = min(orig_end + right, seq_len)
        if end <= start:
            return None
        if (orig_start - left < 0 and left > 0) or (orig_end + right > seq_len and right > 0):
            self.seen.add("clamped")
        self.evaluations += 1
        rows = self.c.query(target_id, start, end, subset_keep=self.subset_keep, **self.query_kw)
        rows = [tuple(int(v) for v in r) for r in rows.tolist()]
        if self.subset_keep is not None:  # apply_subset_filter (:451, subset_filter.rs:93-99): the target's own rows stay
            rows = [r for r in rows if r[0] == target_id or self.subset_keep[r[0]]]
        count, survivors = support(rows, target_id, start, end, self.span_bp, self.merge_distance,
                                   None if self.level == "sequence" else self.key_of, max_entities, self.blacklist)
        return dict(start=start, end=end, left=orig_start - start, right=end - orig_end, count=count, survivors=survivors)

    def single(self, target_id, orig_start, orig_end, label=""):  # refine_single_range (:144-409)
        if orig_end <= orig_start:
            raise ValueError("Invalid range (end must be greater than start)")
        seq_len = self.c.seq_len(target_id)
        ext = max_extension_bp(self.max_extension, max(orig_end - orig_start, 0))
        max_entities = self.compute_max_entities(target_id) if self.level in ("sample", "haplotype") else None
        flanks = build_flanks(ext, self.extension_step)

        def ev(left, right):
            return self.evaluate(target_id, orig_start, orig_end, seq_len, left, right, max_entities)

        def reduce_candidates(cands):
            best = None
            for c in cands:
                if c is not None:
                    best = update_best(best, c)
            return best

        def check_max(c):
            return max_entities is not None and c is not None and c["count"] >= max_entities

        best = ev(0, 0)
        original = best["count"] if best is not None else 0
        if check_max(best):
            self.seen.add("max_at_baseline")
        else:
            c = reduce_candidates([ev(left, 0) for left in flanks if left > 0])
            if c is not None:
                best = update_best(best, c)
            if check_max(best):
                self.seen.add("max_after_left")
            else:
                left_fixed = best["left"] if best is not None else 0
                c = reduce_candidates([ev(left_fixed, right) for right in flanks])
                if c is not None:
                    best = update_best(best, c)
                if check_max(best):
                    self.seen.add("max_after_right")
                else:
                    right_fixed = best["right"] if best is not None else 0
                    c = reduce_candidates([ev(left, right_fixed) for left in flanks])
                    if c is not None:
                        best = update_best(best, c)
        if best is None:
            raise ValueError("No valid flank sizes evaluated")
        if best["left"] > 0:
            self.seen.add("left")
        if best["right"] > 0:
            self.seen.add("right")
        if best["count"] > original:
            self.seen.add("rose")
        if check_max(best):
            self.seen.add("stopped_at_max")
        return dict(target_id=target_id, chrom=self.names[target_id], refined_start=best["start"], refined_end=best["end"],
                    original_start=orig_start, original_end=orig_end, label=label, left_extension=best["left"],
                    right_extension=best["right"], support_count=best["count"], original_support_count=original,
                    survivors=best["survivors"])

    def run(self, loci, labels=None):
        """loci [(target id, start, end)] -> records, in the order of the loci (:116-141)."""
        return [self.single(t, s, e, labels[i] if labels else "") for i, (t, s, e) in enumerate(loci)]

    def text(self, records):
        """(the table, the support file) of main.rs:7817-7861."""
        out = ["#chrom\tstart\tend\tname\toriginal.support\tnew.support\tleft.extension.bp\tright.extension.bp\n"]
        sup = []
        for r in records:
            name = r["label"]
            if name.strip() == "" or name == ".":
                name = "%s:%d-%d" % (r["chrom"], r["original_start"], r["original_end"])
            out.append("%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (r["chrom"], r["refined_start"], r["refined_end"], name, r["original_support_count"],
                                                          r["support_count"], r["left_extension"], r["right_extension"]))
            ents = sorted((self.names[s], lo, hi) for s, lo, hi in r["survivors"])  # :776-780
            for nm, lo, hi in ents:
                sup.append("%s\t%d\t%d\t%s\n" % (nm, lo, hi, name))
        return "".join(out), "".join(sup)


def record_key(r):
    """The fields a library record is compared by."""
    return (r["target_id"], r["refined_start"], r["refined_end"], r["original_start"], r["original_end"], r["left_extension"],
            r["right_extension"], r["support_count"], r["original_support_count"], [tuple(s) for s in r["survivors"]])


# ---- scripted rows with known answers ----------------------------------------------------------------------------------
# Eight sequences; the candidate's target is sequence 0 and its region (1000, 2000) unless a case says otherwise; span_bp
# 100, merge_distance 0.  A row is (query_id, q_first, q_last, target_id, t_first, t_last).  With that region a merged
# interval covers when t_start <= 1000 and t_end >= 2000 (t_end >= 1100 and t_start <= 1900 follow).
N_SEQ = 8
SELF = (0, 1000, 2000, 0, 1000, 2000)
REGION = (0, 1000, 2000)
COVER1 = (1, 500, 1700, 0, 900, 2100)  # covers alone: survivor (1, 500, 1700)


def case(name, rows, want, cand=REGION, span_bp=100, d=0, entity_of=None, max_entities=None, blacklist=None):
    """One call with one candidate; want = (count, survivors)."""
    return dict(name=name, rows=[list(rows)], cands=[cand], span_bp=span_bp, d=d, entity_of=entity_of,
                max_entities=None if max_entities is None else [max_entities], blacklist=blacklist, want=[want])


def scripted_cases():
    A, B = (1, 100, 600, 0, 900, 1400), (1, 600, 1100, 0, 5000, 5600)  # query-adjacent (600 | 600), far apart on the target
    C = (1, 2000, 3000, 0, 800, 2200)                                   # covers alone
    X, Y, Z = (1, 100, 200, 0, 900, 1500), (1, 100, 200, 0, 5000, 6000), (1, 200, 300, 0, 1500, 2100)
    ent = [NO_KEY] * N_SEQ
    ent[1], ent[2], ent[3], ent[5] = 7, 7, 9, 11
    three = [SELF, COVER1, (2, 10, 20, 0, 1000, 2000), (3, 30, 40, 0, 0, 9000)]
    out = [
        # 1: a group of one row; t (900, 2100) covers
        case("one_row", [SELF, COVER1], (1, [(1, 500, 1700)])),
        # 2: neither A (t 900-1400) nor B (t 5000-5600) covers; |A.q_end - B.q_start| = 0 <= 0 merges them by the query
        # axis alone (target distances 3600 and 4700): q (100, 1100), t (900, 5600) covers
        case("query_adjacent", [SELF, A, B], (1, [(1, 100, 1100)])),
        # ... one base apart: not merged, nothing covers
        case("query_gap_1", [SELF, A, (1, 601, 1100, 0, 5000, 5600)], (0, [])),
        # 3: query distances 4400 and 5500; |1500 - 1500| = 0 on the target: q (100, 5600), t (900, 2100) covers
        case("target_adjacent", [SELF, (1, 100, 600, 0, 900, 1500), (1, 5000, 5600, 0, 1500, 2100)], (1, [(1, 100, 5600)])),
        # 4: q (100, 600) and (300, 800) overlap, t (900, 1600) and (1400, 2100) overlap: distances min(300, 700) and
        # min(200, 1200), none <= 0: NOT merged, and neither covers alone
        case("overlap_no_merge", [SELF, (1, 100, 600, 0, 900, 1600), (1, 300, 800, 0, 1400, 2100)], (0, [])),
        # ... at merge_distance 200 the target distance 200 merges them: q (100, 800), t (900, 2100)
        case("overlap_merge_200", [SELF, (1, 100, 600, 0, 900, 1600), (1, 300, 800, 0, 1400, 2100)], (1, [(1, 100, 800)]), d=200),
        # 5: X and Y have q (100, 200) both; Z (200, 300) sorts behind them.  X, Y, Z: X stays alone (distance 100 to Y on
        # the query, thousands on the target), Y absorbs Z (|200 - 200| = 0): t (1500, 6000) starts behind 1000: nothing covers
        case("tie_xy", [SELF, X, Y, Z], (0, [])),
        # ... Y, X, Z: Y stays alone, X absorbs Z: q (100, 300), t (900, 2100) covers
        case("tie_yx", [SELF, Y, X, Z], (1, [(1, 100, 300)])),
        # 6: reverse strand on the query (1700 > 500) and a target interval given backwards: min / max of each
        case("reverse", [SELF, (1, 1700, 500, 0, 900, 2100), (2, 300, 400, 0, 2100, 900)], (2, [(1, 500, 1700), (2, 300, 400)])),
        # 7: a hole is no row; a row whose query is the target is dropped; sequence 1 still covers
        case("hole_and_own_target", [SELF, (HOLE, 0, 0, 0, 0, 0), (0, 5000, 6000, 0, 900, 2100), COVER1], (1, [(1, 500, 1700)])),
        # ... a single row beside a hole: overlaps.len() <= 1 supports nothing, even though the row covers
        case("one_row_and_hole", [COVER1, (HOLE, 0, 0, 0, 0, 0)], (0, [])),
        case("self_only", [SELF], (0, [])),
        # 8
        case("no_rows", [], (0, [])),
        # 9: merge_distance -1 merges nothing: only C covers, the hull is C's; at 0, A + B merge (case 2) and cover too,
        # C stays apart (query distance 900, target distances 4800 and 1300): hull (100, 3000)
        case("no_merge", [SELF, A, B, C], (1, [(1, 2000, 3000)]), d=-1),
        case("no_merge_control", [SELF, A, B, C], (1, [(1, 100, 3000)])),
        # 10: span 5000 > the region: effective_span 1000, thresholds (2000, 1000): the exact fit covers
        case("span_beyond_region", [SELF, (1, 5, 6, 0, 1000, 2000)], (1, [(1, 5, 6)]), span_bp=5000),
        # 11: span -5 counts as 0
        case("negative_span", [SELF, (1, 5, 6, 0, 1000, 2000)], (1, [(1, 5, 6)]), span_bp=-5),
        # 12: with start < end the first two inequalities bind (t_start <= 1000, t_end >= 2000) ...
        case("cover_exact", [SELF, (1, 5, 6, 0, 1000, 2000)], (1, [(1, 5, 6)])),
        case("cover_miss_start", [SELF, (1, 5, 6, 0, 1001, 2000)], (0, [])),
        case("cover_miss_end", [SELF, (1, 5, 6, 0, 1000, 1999)], (0, [])),
        # ... and with a region handed over backwards, (2000, 1000), effective_span is 0 and the other two bind:
        # t_end >= start = 2000 and t_start <= end = 1000 (t_start <= 2000 and t_end >= 1000 follow)
        case("cover_inverted_exact", [SELF, (1, 5, 6, 0, 1000, 2000)], (1, [(1, 5, 6)]), cand=(0, 2000, 1000)),
        case("cover_miss_left_threshold", [SELF, (1, 5, 6, 0, 1000, 1999)], (0, []), cand=(0, 2000, 1000)),
        case("cover_miss_right_threshold", [SELF, (1, 5, 6, 0, 1001, 2000)], (0, []), cand=(0, 2000, 1000)),
        # 13: the hull of sequence 1 is [500, 1700], both ends inclusive, and so are the ranges'
        case("bl_end_at_lo", [SELF, COVER1], (0, []), blacklist={1: [(100, 500)]}),
        case("bl_end_before_lo", [SELF, COVER1], (1, [(1, 500, 1700)]), blacklist={1: [(100, 499)]}),
        case("bl_start_at_hi", [SELF, COVER1], (0, []), blacklist={1: [(1700, 1800)]}),
        case("bl_start_behind_hi", [SELF, COVER1], (1, [(1, 500, 1700)]), blacklist={1: [(1701, 1800)]}),
        case("bl_overlapping_miss", [SELF, COVER1], (1, [(1, 500, 1700)]), blacklist={1: [(1800, 1900), (200, 499), (100, 300)]}),
        case("bl_overlapping_hit", [SELF, COVER1], (0, []), blacklist={1: [(1800, 1900), (200, 500), (100, 300)]}),
        case("bl_other_sequence", [SELF, COVER1], (1, [(1, 500, 1700)]), blacklist={2: [(0, 9000)]}),
        # 14: sequences 1 and 2 are entity 7, sequence 3 entity 9: three survivors, two entities
        case("two_of_one_entity", three, (2, [(1, 500, 1700), (2, 10, 20), (3, 30, 40)]), entity_of=ent),
        # 15: sequence 4 has no key: a survivor that counts nothing
        case("no_key", [SELF, COVER1, (4, 10, 20, 0, 1000, 2000)], (1, [(1, 500, 1700), (4, 10, 20)]), entity_of=ent),
        # 16: entities 7, 9, 11 under max_entities 2: the count is clamped, every survivor is kept
        case("clamp", three + [(5, 50, 60, 0, 1000, 2000)], (2, [(1, 500, 1700), (2, 10, 20), (3, 30, 40), (5, 50, 60)]), entity_of=ent,
             max_entities=2),
    ]
    # every case once more as one call of many candidates (those without a blacklist or entities of their own)
    plain = [c for c in out if c["entity_of"] is None and c["blacklist"] is None and c["span_bp"] == 100 and c["d"] == 0]
    out.append(dict(name="batch", rows=[c["rows"][0] for c in plain], cands=[c["cands"][0] for c in plain], span_bp=100, d=0, entity_of=None,
                    max_entities=None, blacklist=None, want=[c["want"][0] for c in plain]))
    return out


def rows_array(per_candidate):
    """[[row, ...] per candidate] -> (structured rows, offsets) for impg_amd.support_rows."""
    import numpy as np

    from impg_amd import _lib
    flat = [r for rows in per_candidate for r in rows]
    a = np.array(flat, dtype=_lib.INTERVAL_DTYPE) if flat else np.zeros(0, dtype=_lib.INTERVAL_DTYPE)
    off = np.concatenate([[0], np.cumsum([len(r) for r in per_candidate])]).astype(np.uint64)
    return a, off


def support_batch(per_candidate, cands, span_bp, d, entity_of=None, max_entities=None, blacklist=None):
    """The restatement over a batch: ([count], [survivors])."""
    key_of = None if entity_of is None else (lambda s: None if entity_of[s] == NO_KEY else entity_of[s])
    res = [support(rows, t, s, e, span_bp, d, key_of, None if max_entities is None else max_entities[i], blacklist)
           for i, (rows, (t, s, e)) in enumerate(zip(per_candidate, cands))]
    return [r[0] for r in res], [r[1] for r in res]


# ---- the end-to-end runs of test_refine_cpu.py / test_gpu_refine.py ------------------------------------------------------
E2E_SEED = 20261019
E2E_OPTS = dict(span_bp=500, max_extension=3000, extension_step=500, merge_distance=5000)
# (target, start) of loci of 2 kb on the synthetic PAF of that seed, chosen with the restatement so that the search has
# something to find: support that rises with a left flank, with a right flank, with both, loci that reach their
# max_entities at the baseline, after the left and after the right pass, and loci at the ends of their sequences
E2E_PICKED = [(7, 71844), (11, 135290), (12, 55811), (3, 126587), (5, 28543), (18, 127478), (16, 89630), (19, 51938), (17, 58007),
              (4, 123450), (4, 72879), (14, 152474), (1, 74495), (2, 31196), (19, 54356), (7, 81021), (12, 24535), (18, 159279),
              (0, 166296), (10, 13605), (15, 131666), (1, 72804), (10, 174549), (8, 157203), (4, 52219), (3, 160434),
              (0, 700), (3, 300), (5, 197100), (9, 196500), (13, 0), (6, 198000)]


def e2e_loci(c, n=40, length=2000):
    """n loci of `length` bp: the picked ones, then some spread over the sequences."""
    loci = [(t, s, s + length) for t, s in E2E_PICKED]
    n_seq = c.num_seqs()
    for k in range(n - len(loci)):
        t = (k * 7 + 2) % n_seq
        s = ((k * 7919 + 13) * 997) % (c.seq_len(t) - 3 * length) + length
        loci.append((t, s, s + length))
    return loci
