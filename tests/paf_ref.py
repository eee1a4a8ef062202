"""A Python model of the device PAF route (impg_amd/csrc/paf_device.inc) and a generator of chains of one-op rows.

The merge is the device BEDPE route's (tests/bedpe_ref.py: one pairwise test between neighbours of the sorted order).  What
PAF adds is the merged CIGAR, and the model computes it as the device does, without a fold over the run: a run's rows in
text order, one element per row (the join's gap ops, then the row's ops), a four-field summary per element, a suffix scan
of the summaries for the bases a group gains from the elements behind it, and every element printing the groups that start
in it.  tests/test_paf_ref_cpu.py holds the model against the oracle's restatement of merge_adjusted_intervals +
output_results_paf byte for byte; the GPU tests hold the device against both and against the model's counters.
"""
import numpy as np

from tests.bedpe_ref import E_INVALID, E_UNSUPPORTED, OP_LEN_MASK, U32, Refused, fmt_f32, i32, join_kind

OP_CHARS = "=XIDM"

COUNTERS = ("paf_rows", "paf_runs", "paf_joins_contiguous", "paf_joins_gap", "paf_ops_read", "paf_ops_printed", "paf_through_rows",
            "paf_text_bytes")


def new_counters():
    c = dict.fromkeys(COUNTERS, 0)
    c.update(multi_runs=0, reverse_multi_runs=0, reverse_through_rows=0)  # (the model's own tallies, beyond the handle's counters)
    return c


def element_summary(ops):
    """(lead_code, lead_len, all_same, last_code) of a non-empty list of (code, length)."""
    code = ops[0][0]
    k = 0
    ln = 0
    while k < len(ops) and ops[k][0] == code:
        ln += ops[k][1]
        k += 1
    return code, ln, k == len(ops), ops[-1][0]


def compose(a, b):
    """The (lead_code, lead_len, all_same) of the concatenation of two strings of ops from those of its halves."""
    through = a[2] and b[0] == a[0]
    return a[0], a[1] + (b[1] if through else 0), through and b[2]


def run_cigar(elements, tally=None):
    """The printed ops of a run of two rows or more: elements[t] = [(code, length), ...] in text order."""
    sums = [element_summary(e) for e in elements]
    n = len(elements)
    suffix = [None] * (n + 1)  # suffix[t]: the summary of elements t .. n-1
    for t in range(n - 1, -1, -1):
        suffix[t] = sums[t][:3] if suffix[t + 1] is None else compose(sums[t][:3], suffix[t + 1])
    out = []
    for t, ops in enumerate(elements):
        starts = t == 0 or sums[t - 1][3] != sums[t][0]
        ext = suffix[t + 1][1] if suffix[t + 1] is not None and suffix[t + 1][0] == sums[t][3] else 0
        groups = []
        for code, ln in ops:
            if groups and groups[-1][0] == code:
                groups[-1][1] += ln
            else:
                groups.append([code, ln])
        groups[-1][1] += ext
        if not starts:
            groups = groups[1:]  # (it started in an element before this one, which printed it)
        if not groups and tally is not None:
            tally["paf_through_rows"] += 1
        out += [(c, ln) for c, ln in groups]
    return out


def paf_range(rows, cigars, d, range_name, seq_name, seq_len, seq_shift=None, original=False, transitive=False, min_output_length=-1,
              counters=None):
    """The PAF text of one range.  rows / cigars: what the query returns with store_cigar, the range itself first (rows:
    (query_id, q_first, q_last, target_id, t_first, t_last); cigars: packed op arrays).  seq_name(id) / seq_len(id) /
    seq_shift(id): the printed name, the printed length and the offset added to the coordinates; original: the lengths
    print as 0.  counters: a new_counters() dict, added to."""
    c = counters if counters is not None else new_counters()
    rows = [tuple(int(v) for v in r) for r in rows]
    keep = [k for k, r in enumerate(rows) if transitive or min_output_length < 0 or abs(r[2] - r[1]) >= min_output_length]
    if not keep:
        raise Refused(E_INVALID, "no result row to drop")
    keep = keep[1:]
    rows = [rows[k] for k in keep]
    ops = [[(int(v) >> 29, int(v) & OP_LEN_MASK) for v in cigars[k]] for k in keep]
    if any(not o for o in ops):
        raise Refused(E_UNSUPPORTED, "a result row without CIGAR")
    order = list(range(len(rows)))
    if d >= 0:
        if len(rows) >= 2 and any(r[4] > r[5] for r in rows):
            raise Refused(E_INVALID, "Target intervals should always be in forward!")

        def key(k):
            r = rows[k]
            af = r[1] < r[2]  # strict
            return (r[0], af, r[1] if af else r[2], r[3], r[4])
        order.sort(key=key)
    c["paf_rows"] += len(rows)
    c["paf_ops_read"] += sum(len(o) for o in ops)
    joins = [(0, 0, 0)] * len(order)
    for k in range(1, len(order)):
        if d >= 0:
            joins[k] = join_kind(rows[order[k - 1]], rows[order[k]], d)
    out = []
    k = 0
    while k < len(order):
        e = k + 1
        while e < len(order) and joins[e][0]:
            e += 1
        members = [order[i] for i in range(k, e)]
        head, tail = rows[members[0]], rows[members[-1]]
        f = head[1] <= head[2]
        if len(members) == 1:
            printed = ops[members[0]]  # raw: nothing is fused without a join
        else:
            # text order: sorted when forward, reverse sorted when reverse; the gap in front of text row t is the join
            # between the two sorted neighbours, [qd I] [td D] in that order on both strands
            gaps = [joins[i][1:] for i in range(k + 1, e)]
            text_members, text_gaps = (members, gaps) if f else (members[::-1], gaps[::-1])
            elements = []
            for t, r in enumerate(text_members):
                el = []
                if t:
                    qd, td = text_gaps[t - 1]
                    el += ([(2, qd)] if qd > 0 else []) + ([(3, td)] if td > 0 else [])
                elements.append(el + ops[r])
            through_before = c["paf_through_rows"]
            printed = run_cigar(elements, c)
            c["multi_runs"] += 1
            c["reverse_multi_runs"] += not f
            c["reverse_through_rows"] += 0 if f else c["paf_through_rows"] - through_before
            for i in range(k + 1, e):
                c["paf_joins_contiguous" if joins[i][0] == 1 else "paf_joins_gap"] += 1
        c["paf_ops_printed"] += len(printed)
        m = sum(ln for code, ln in printed if code in (0, 4)) & U32
        x = sum(ln for code, ln in printed if code == 1) & U32
        ibp = sum(ln for code, ln in printed if code == 2) & U32
        dbp = sum(ln for code, ln in printed if code == 3) & U32
        ni = sum(1 for code, _ in printed if code == 2)
        nd = sum(1 for code, _ in printed if code == 3)
        box = (head[1], tail[2], head[4], tail[5]) if f else (tail[1], head[2], tail[4], head[5])
        bf = box[0] <= box[1]
        first, last = (box[0], box[1]) if bf else (box[1], box[0])
        gi = fmt_f32(i32(m), i32(m + x + ni + nd))
        bi = fmt_f32(i32(m), i32(m + ((x + ibp + dbp) & U32)))
        qo = seq_shift(head[0]) if seq_shift else 0
        to = seq_shift(head[3]) if seq_shift else 0
        cg = "".join("%d%s" % (ln, OP_CHARS[code] if code < 5 else "?") for code, ln in printed)
        out.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\tgi:f:%s\tbi:f:%s\tcg:Z:%s\tan:Z:%s\n" % (
            seq_name(head[0]), 0 if original else seq_len(head[0]), (first + qo) & U32, (last + qo) & U32, "+" if bf else "-",
            seq_name(head[3]), 0 if original else seq_len(head[3]), (box[2] + to) & U32, (box[3] + to) & U32, i32(m), i32(m + x + ibp + dbp), gi, bi,
            cg, range_name))
        c["paf_runs"] += 1
        k = e
    text = "".join(out)
    c["paf_text_bytes"] += len(text.encode())
    return text


# ---- chains of one-op rows ---------------------------------------------------------------------------------------------
CHAIN_NAMES = ["c0", "c1", "c2"]
CHAIN_SEQ_LEN = 9000
CHAIN_GAPS = [0, 0, 0, 1, 3]


def chain_paf(seed, n_chains=6, n_blocks=14, prefix=""):
    """Chains of records of ONE op each that tile a query and a target sequence, contiguous or a few bases apart, on both
    strands; a block keeps the code of the block before it six times in ten, so that groups run through whole rows.
    Returns (text, ranges as (seq id, start, end)); the sequences are called prefix + CHAIN_NAMES[seq id]."""
    rng = np.random.default_rng(1000 + seed)
    lines, chains = [], []
    for ch in range(n_chains):
        t = int(rng.integers(0, 3))
        q = (t + 1 + int(rng.integers(0, 2))) % 3
        reverse = ch % 2 == 1
        tpos = 200 + ch * 1300 + int(rng.integers(0, 40))
        qlo = 150 + ch * 1300 + int(rng.integers(0, 40))
        qpos = qlo + 1250 if reverse else qlo
        t0 = tpos
        code = "="
        for _ in range(n_blocks):
            if rng.random() >= 0.6:
                code = "=XMD=X"[int(rng.integers(0, 6))]
            n = int(rng.integers(1, 30))
            td, qd = (n, 0) if code == "D" else (n, n)
            gt, gq = (CHAIN_GAPS[int(rng.integers(0, 5))] for _ in range(2))
            if reverse and rng.random() < 0.5:
                gq = 0  # (a reverse-strand gap join needs the query axis contiguous)
            qs, qe = (qpos - qd, qpos) if reverse else (qpos, qpos + qd)
            lines.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%d%s" % (
                prefix + CHAIN_NAMES[q], CHAIN_SEQ_LEN, qs, qe, "-" if reverse else "+", prefix + CHAIN_NAMES[t], CHAIN_SEQ_LEN, tpos, tpos + td, td,
                td + qd, n, code))
            tpos += td + gt
            qpos = qs - gq if reverse else qe + gq
        chains.append((t, t0, tpos))
    order = rng.permutation(len(lines))
    text = "\n".join(lines[i] for i in order) + "\n"
    ranges = [(0, 0, CHAIN_SEQ_LEN), (1, 0, CHAIN_SEQ_LEN), (2, 0, CHAIN_SEQ_LEN)] + [(t, max(0, a - 30), b + 30) for t, a, b in chains[:2]]
    return text, ranges


def pack(cg):
    """'5=2I' -> packed uint32 ops"""
    out, num = [], ""
    for ch in cg:
        if ch.isdigit():
            num += ch
        else:
            out.append(int(num) | OP_CHARS.index(ch) << 29)
            num = ""
    return np.array(out, dtype=np.uint32)
