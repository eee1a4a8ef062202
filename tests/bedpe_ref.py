"""A Python model of the device BEDPE route (impg_amd/csrc/bedpe_device.hip) and a dense generator of tiling PAFs.

The model works as the device does, not as the reference's fold does: a 10-field summary per row, one pairwise test
between neighbours of the sorted order, sums with local corrections at the joins, and gi:f / bi:f formatted from
f32 quotients by integer arithmetic.  tests/test_bedpe_ref_cpu.py holds it against the oracle's restatement of
merge_adjusted_intervals + output_results_bedpe byte for byte; the GPU tests then hold the device against both and
against the model's counters.
"""
import numpy as np

U32 = 0xFFFFFFFF
OP_LEN_MASK = (1 << 29) - 1

E_INVALID, E_UNSUPPORTED = "invalid", "unsupported"


class Refused(Exception):
    """A range the route refuses: kind is E_INVALID or E_UNSUPPORTED."""

    def __init__(self, kind, msg):
        Exception.__init__(self, msg)
        self.kind = kind


def i32(v):
    v &= U32
    return v - (1 << 32) if v >> 31 else v


def summarize(ops):
    """{m, x, ibp, dbp, ni, nd, ii, dd, first, last} of one row's packed ops (u32 sums, wrapping)."""
    s = dict(m=0, x=0, ibp=0, dbp=0, ni=0, nd=0, ii=0, dd=0, first=7, last=7, n=len(ops))
    before = 7
    for k, op in enumerate(int(v) for v in ops):
        code, ln = op >> 29, op & OP_LEN_MASK
        if code in (0, 4):
            s["m"] = (s["m"] + ln) & U32
        elif code == 1:
            s["x"] = (s["x"] + ln) & U32
        elif code == 2:
            s["ibp"] = (s["ibp"] + ln) & U32
            s["ni"] += 1
            s["ii"] += before == 2
        elif code == 3:
            s["dbp"] = (s["dbp"] + ln) & U32
            s["nd"] += 1
            s["dd"] += before == 3
        if k == 0:
            s["first"] = code
        s["last"] = code
        before = code
    return s


def join_kind(a, b, d):
    """Does row b continue the run of row a, its predecessor in sorted order?  (0 | 1 contiguous | 2 gap, qd, td).
    Rows are (query_id, q_first, q_last, target_id, t_first, t_last)."""
    f = a[1] <= a[2]
    if a[0] != b[0] or a[3] != b[3] or f != (b[1] <= b[2]):
        return 0, 0, 0
    qd = i32(b[1] - a[2]) if f else i32(a[1] - b[2])
    td = i32(b[4] - a[5]) if f else i32(a[4] - b[5])
    if qd == 0 and td == 0:
        return 1, qd, td
    q_over = qd < 0 if f else qd > 0
    if not q_over and td >= 0 and qd >= 0 and (qd > 0 or td > 0) and qd <= d and td <= d:
        return 2, qd, td
    return 0, 0, 0


def fmt_f32(m, den):
    """(f32)m / (f32)den as format!("{:.6}") prints it, trailing zeros and a trailing '.' trimmed; m, den: i32."""
    with np.errstate(all="ignore"):
        v = np.float32(m) / np.float32(den)
    if np.isnan(v):
        return "NaN"
    sign = "-" if np.signbit(v) else ""
    if np.isinf(v):
        return sign + "inf"
    scaled = int(np.rint(np.float64(abs(v)) * 1e6))  # exact product, ties to even
    ip, fr = divmod(scaled, 1000000)
    out = sign + str(ip)
    if fr:
        out += "." + ("%06d" % fr).rstrip("0")
    return out


COUNTERS = ("bedpe_rows", "bedpe_runs", "bedpe_joins_contiguous", "bedpe_joins_gap", "bedpe_fused_ops", "bedpe_summary_ops",
            "bedpe_text_bytes")


def new_counters():
    c = dict.fromkeys(COUNTERS, 0)
    c.update(joins_reverse=0, fused_at_joins=0, fused_in_rows=0)  # (the model's own tallies, beyond the handle's counters)
    return c


def bedpe_range(rows, cigars, d, range_name, seq_name, seq_shift=None, transitive=False, min_output_length=-1, counters=None):
    """The BEDPE text of one range.  rows / cigars: what the query returns with store_cigar, the range itself first
    (rows: sequences of (query_id, q_first, q_last, target_id, t_first, t_last); cigars: packed op arrays).  seq_name(id)
    / seq_shift(id): the printed name and the offset added to its coordinates.  counters: a new_counters() dict, added to."""
    c = counters if counters is not None else new_counters()
    rows = [tuple(int(v) for v in r) for r in rows]
    keep = [k for k, r in enumerate(rows) if transitive or min_output_length < 0 or abs(r[2] - r[1]) >= min_output_length]
    if not keep:
        raise Refused(E_INVALID, "no result row to drop")
    keep = keep[1:]
    rows = [rows[k] for k in keep]
    sums = [summarize(cigars[k]) for k in keep]
    if any(s["n"] == 0 for s in sums):
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
    c["bedpe_rows"] += len(rows)
    c["bedpe_summary_ops"] += sum(s["n"] for s in sums)
    # heads
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
        tot = dict(m=0, x=0, ibp=0, dbp=0, ni=0, nd=0)
        if len(members) == 1:
            for name in tot:
                tot[name] = sums[members[0]][name]
        else:
            for i in members:
                s = sums[i]
                for name in ("m", "x", "ibp", "dbp"):
                    tot[name] += s[name]
                tot["ni"] += s["ni"] - s["ii"]
                tot["nd"] += s["nd"] - s["dd"]
                c["fused_in_rows"] += s["ii"] + s["dd"]
            for i in range(k + 1, e):
                kind, qd, td = joins[i]
                a, b = (sums[order[i - 1]], sums[order[i]]) if f else (sums[order[i]], sums[order[i - 1]])
                seq = [a["last"]] + ([2] if qd > 0 else []) + ([3] if td > 0 else []) + [b["first"]]
                fi = sum(1 for u, v in zip(seq, seq[1:]) if u == v == 2)
                fd = sum(1 for u, v in zip(seq, seq[1:]) if u == v == 3)
                tot["ibp"] += qd
                tot["dbp"] += td
                tot["ni"] += (qd > 0) - fi
                tot["nd"] += (td > 0) - fd
                c["fused_at_joins"] += fi + fd
                c["bedpe_joins_contiguous" if kind == 1 else "bedpe_joins_gap"] += 1
                c["joins_reverse"] += not f
        box = (head[1], tail[2], head[4], tail[5]) if f else (tail[1], head[2], tail[4], head[5])
        bf = box[0] <= box[1]
        first, last = (box[0], box[1]) if bf else (box[1], box[0])
        m, x, ibp, dbp, ni, nd = (tot[n] & U32 for n in ("m", "x", "ibp", "dbp", "ni", "nd"))
        gi = fmt_f32(i32(m), i32(m + x + ni + nd))
        bi = fmt_f32(i32(m), i32(m + ((x + ibp + dbp) & U32)))
        qo = seq_shift(head[0]) if seq_shift else 0
        to = seq_shift(head[3]) if seq_shift else 0
        out.append("%s\t%d\t%d\t%s\t%d\t%d\t%s\t0\t%s\t+\tgi:f:%s\tbi:f:%s\n" % (
            seq_name(head[0]), (first + qo) & U32, (last + qo) & U32, seq_name(head[3]), (box[2] + to) & U32, (box[3] + to) & U32,
            range_name, "+" if bf else "-", gi, bi))
        c["bedpe_runs"] += 1
        k = e
    text = "".join(out)
    c["bedpe_fused_ops"] = c["fused_at_joins"] + c["fused_in_rows"]
    c["bedpe_text_bytes"] += len(text.encode())
    return text


# ---- dense tiling PAFs -------------------------------------------------------------------------------------------------
DENSE_CIGARS = ["20=", "3I17=", "17=3I", "2D18=", "18=2D", "5=2I3I10=", "4D4D12=", "2I", "3D", "6=2X4M", "1I1D10=1D1I", "0=5=", "1=127X"]
DENSE_GAPS = [0, 1, 2, 5, -1]
DENSE_NAMES = ["d0", "d1", "d2"]
DENSE_SEQ_LEN = 9000


def cigar_spans(cg):
    td = qd = 0
    num = ""
    for ch in cg:
        if ch.isdigit():
            num += ch
            continue
        n = int(num)
        num = ""
        if ch in "=XM":
            td += n
            qd += n
        elif ch == "D":
            td += n
        elif ch == "I":
            qd += n
    return td, qd


def dense_paf(seed, n_chains=6, n_blocks=12, prefix=""):
    """Chains of blocks that tile a query and a target sequence, consecutive blocks 0, 1, 2, 5 or -1 bases apart on each
    axis, on both strands, CIGARs from DENSE_CIGARS; records shuffled.  Returns (text, ranges as (seq id, start, end));
    the sequences are called prefix + DENSE_NAMES[seq id]."""
    rng = np.random.default_rng(seed)
    lines = []
    chains = []
    for ch in range(n_chains):
        t = int(rng.integers(0, 3))
        q = (t + 1 + int(rng.integers(0, 2))) % 3
        reverse = ch % 2 == 1
        tpos = 200 + ch * 1300 + int(rng.integers(0, 40))
        qlo = 150 + ch * 1300 + int(rng.integers(0, 40))
        qpos = qlo + 1250 if reverse else qlo  # reverse: the query runs down while the target runs up
        t0 = tpos
        for _ in range(n_blocks):
            cg = DENSE_CIGARS[int(rng.integers(0, len(DENSE_CIGARS)))]
            td, qd = cigar_spans(cg)
            gt, gq = (DENSE_GAPS[int(rng.integers(0, 5))] for _ in range(2))
            if reverse and rng.random() < 0.5:
                gq = 0  # (a reverse-strand gap join needs the query axis contiguous)
            qs, qe = (qpos - qd, qpos) if reverse else (qpos, qpos + qd)
            lines.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%s" % (
                prefix + DENSE_NAMES[q], DENSE_SEQ_LEN, qs, qe, "-" if reverse else "+", prefix + DENSE_NAMES[t], DENSE_SEQ_LEN, tpos, tpos + td, td, td + qd, cg))
            tpos += td + gt
            qpos = qs - gq if reverse else qe + gq
        chains.append((t, t0, tpos))
    order = rng.permutation(len(lines))
    text = "\n".join(lines[i] for i in order) + "\n"
    t, a, b = chains[int(rng.integers(0, n_chains))]
    cut = int(rng.integers(3, 40))
    ranges = [(0, 0, DENSE_SEQ_LEN), (t, max(0, a - 30), b + 30), (t, a + cut, max(a + cut + 120, b - cut))]
    return text, ranges
