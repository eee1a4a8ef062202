"""tests/lookup_gen.py checked without a GPU: its case list reaches every path and edge of the lookup's wide-window emit that
tests/test_gpu_lookup_paths.py is about, and the oracle agrees with the fixtures' arithmetic (a ladder range's window is
exactly [a, b), every entry a hit; the umbrella ladder's empty entries are what a plain and a transitive window disagree on)."""
import pytest

from oracle import oracle as o
from tests import lookup_gen as lg

_built = {}


def built(case):
    """(oracle index, {target: ranks}) of a case's fixture; ranks only under ORDER_COITREES (see lookup_gen: where a rank comes from)."""
    key = (case.n, case.n2)
    if key not in _built:
        c = o.OracleIndex(paf_text=lg.paf(case.n, case.n2), bidirectional=False, preparse=True)
        ranks = {}
        if case.n:
            ranks["T"] = lg.visit_ranks(c, c.seq_id("T"), case.n)
        if case.n2:
            m = len(lg.umbrella_entries(case.n2))
            c2 = o.OracleIndex(paf_text=lg.paf(m), bidirectional=False, preparse=True)
            ranks["T2"] = lg.visit_ranks(c2, c2.seq_id("T"), m)
        _built[key] = (c, ranks)
    return _built[key]


def all_plans(case, cap=lg.WIDE_CAP, bins=lg.WIDE_BINS):
    c, ranks = built(case)
    out = []
    for kw in case.modes:
        p, w = lg.plans(case, ranks, bool(kw.get("transitive")), cap, bins)
        out += list(zip(case.ranges, p, w))
    return out


def test_shift_rule_is_the_smallest_shift():
    """The kernel's two-step rule and the model's definition are the same number -- and differ from the first step alone
    where dom >> shift == bins with low bits left over, first at dom = bins * 2^k + 1, k >= 1 (bins + 1 itself is still the
    first step's: 1025 >> 0 > 1024)."""
    for bins in (2, 3, 4, 8, 16, 100, 1000, 1024):
        for dom in list(range(1, 20000)) + [bins * (1 << k) + d for k in range(0, 16) for d in (-1, 0, 1)]:
            if dom < 1:
                continue
            s = lg.bin_shift(dom, bins)
            assert s == lg.kernel_shift(dom, bins), (dom, bins)
            assert (dom - 1) >> s < bins and (s == 0 or (dom - 1) >> (s - 1) >= bins)
    assert lg.bin_shift(1024) == 0 and lg.bin_shift(1025) == 1
    for k in range(1, 6):  # the first step alone leaves the top key in bin `bins`
        dom = 1024 * (1 << k) + 1
        first = 0
        while (dom >> first) > 1024:
            first += 1
        assert first == k and (dom - 1) >> first == 1024 and lg.bin_shift(dom) == k + 1


@pytest.mark.parametrize("name", list(lg.CASES))
def test_oracle_counts_are_the_windows(name):
    """A ladder range's count is b - a under both hit tests; a T2 range's is the model's hits, less the empty entries a plain
    window hits (they project to nothing).  Under ORDER_COITREES the rows come out by ascending model rank."""
    case = lg.CASES[name]
    c, ranks = built(case)
    seen = set()
    for kw in case.modes[:2]:
        tr = bool(kw.get("transitive"))
        for t, s, e in case.ranges:
            if (t, s, e, tr) in seen:
                continue
            seen.add((t, s, e, tr))
            ent = lg.entries_of(case, t)
            lo, ub, hits = lg.window(ent, s, e, tr)
            rows = c.query(c.seq_id(t), s, e, **kw)[1:]
            if t == "T":
                a, b = (s - 100) // 20, (e - 101) // 20 + 1
                assert (s, e) == lg.ladder_range(a, b) and (lo, ub) == (a, b) and len(hits) == b - a
                assert len(rows) == b - a, (name, t, s, e, kw)
            else:
                assert lo == 0
                live = [i for i in hits if ent[i][0] < ent[i][1]]
                assert len(rows) == len(live), (name, t, s, e, kw)
                empties = [i for i in hits if ent[i][0] == ent[i][1]]  # (only the closed test hits an empty entry)
                assert not (tr and empties)
                hits = live
            if case.order == lg.COITREES:  # the oracle visits the hits by ascending rank
                at = {ent[i][0]: ranks[t][i] for i in hits if i or t == "T"}
                qu = c.seq_id("qU")  # (the umbrella's row is clipped to the range: known by its query)
                got = [ranks[t][0] if q == qu else at[100 + (int(x) - 100) // 20 * 20] for q, x in zip(rows["query_id"], rows["t_first"])]
                assert got == sorted(got), (name, t, s, e, kw)


def test_case_list_reaches_every_path_and_edge():
    reached = {}
    for case in lg.CASES.values():
        for cap, bins in case.limits:
            for r, p, (lo, ub, h) in all_plans(case, cap, bins):
                reached.setdefault(case.name, []).append((cap, bins, r, p, lo, ub, h))
    every = [x for v in reached.values() for x in v]
    default = [x for x in every if x[:2] == (lg.WIDE_CAP, lg.WIDE_BINS)]
    # every path; every counter rises somewhere
    assert {x[3].path for x in default} == {"lane", "single", "grouped"}  # (overflow at the natural limits needs a 4 * 10^6-entry segment)
    assert {x[3].path for x in every} == {"lane", "single", "grouped", "overflow"}
    total = lg.counters_of([x[3] for x in every])
    assert all(total[k] > 0 for k in lg.COUNTERS), total
    # the width boundary: (lo & 3) + width of 64 (narrow) and 65 (wide) for every lo & 3 on the ladder, and on T2 (every window
    # starts at its segment's first entry, place N_MAIN of the entry array)
    wb = [x for x in reached["width_boundary"]]
    for t in ("T", "T2"):
        edge = {(lo & 3, (lo & 3) + ub - lo, p.path != "lane") for _, _, r, p, lo, ub, h in wb if r[0] == t}
        for m in ((0, 1, 2, 3) if t == "T" else (lg.N_MAIN & 3,)):
            assert (m, 64, False) in edge and (m, 65, True) in edge, (t, m)
        assert all(wide == (s > 64) for _, s, wide in edge)
    # hit counts of one pass: the P2 floor (64 / 65), a block's width (255 / 256 / 257), the buffer (4095 / 4096 one pass, 4097 groups)
    singles = {h for _, _, r, p, lo, ub, h in reached["hit_counts"] if p.path == "single"}
    assert set(lg.HIT_COUNTS) <= singles and any(h < 64 for h in singles) and {2, 3, 4, 5} <= singles
    grouped = [x for x in default if x[3].path == "grouped"]
    assert {4097, 8193} <= {x[6] for x in grouped}
    full = [x[3] for x in reached["groups_8193"] if (x[4], x[5]) == (0, 8193)]
    assert full and all(p.shift == 4 and p.groups == (4096, 4096, 1) and p.passes == 3 for p in full)
    assert any(g == lg.WIDE_CAP for x in grouped for g in x[3].groups)  # a group that closes at exactly the buffer
    assert any(x[5] == 8193 and x[4] > 0 for x in reached["groups_8193"]) and any(x[5] == 4097 for x in reached["groups_8193"])
    # the shift edge: key domains of 1024 * 2^k + 1 whose top key is among the hits, under both order policies
    for order, want in ((lg.COITREES, {1025, 2049, 4097, 8193}), (lg.SORTED, {1025, 2049, 4097, 8193})):
        doms = set()
        for case in lg.CASES.values():
            if case.order != order or case.limits != lg.DEFAULT:
                continue
            c, ranks = built(case)
            for r, p, (lo, ub, h) in all_plans(case):
                if p.path == "lane":
                    continue
                dom = lg.key_domain(lo, ub, order, lg.max_seg(case))
                off = lg.seg_offset(case, r[0])
                keys = lg.hit_ranks(lo - off, list(range(lo - off, ub - off)), order, ranks.get(r[0]))
                if dom - 1 in keys:
                    doms.add(dom)
        assert want <= doms and 1024 in doms, (order, sorted(doms))
    # ... and under ORDER_COITREES, for each of the five ladders, both named ranges: the full cover, and the last 100 entries -- one
    # pass, the top key n - 1 among its hits
    for n in (1024, 1025, 2049, 4097, 8193):
        found = set()
        for case in lg.CASES.values():
            if case.order != lg.COITREES or case.n != n or case.n2 or case.limits != lg.DEFAULT:
                continue
            c, ranks = built(case)
            for r, p, (lo, ub, h) in all_plans(case):
                if (lo, ub) in ((0, n), (n - 100, n)) and n - 1 in ranks["T"][lo:ub] and lg.key_domain(lo, ub, lg.COITREES, lg.max_seg(case)) == n:
                    found.add((ub - lo, p.path))
        assert (100, "single") in found and (n, "single" if n <= lg.WIDE_CAP else "grouped") in found, (n, found)
    # lowered limits: one batch with a single pass, groups of >= 3 passes and an overflow window -- under one setting
    for name in ("lowered_limits", "small_batch"):
        cap, bins = lg.CASES[name].limits[0]
        low = [x[3] for x in reached[name] if x[:2] == (cap, bins)]
        assert {"single", "overflow"} <= {p.path for p in low} and any(p.passes >= 3 for p in low), name
        assert all(x[3].path in ("single", "lane") for x in reached[name] if x[:2] == (lg.WIDE_CAP, lg.WIDE_BINS))
    assert any(p.passes >= 3 for p in [x[3] for x in reached["lowered_limits_sorted"]])
    # more listed windows than the emit grid has blocks
    mw = lg.CASES["many_windows"]
    assert len(mw.ranges) == 5000 and sum(1 for x in reached["many_windows"][:5000] if x[3].path != "lane") > lg.EMIT_GRID
    # the small-batch path takes the batch: plain, <= 64 ranges, the sum of their targets' segments <= 2^18
    sb = lg.CASES["small_batch"]
    assert len(sb.ranges) <= 30 and len(sb.ranges) <= lg.SMALL_RANGES and sb.modes == (dict(),)
    assert sum(len(lg.entries_of(sb, t)) for t, _, _ in sb.ranges) <= lg.SMALL_PAIRS
    assert all(x[3].path != "lane" for x in reached["small_batch"])
    # empty entries inside wide windows: hit by the plain window, not by the transitive one
    fz = lg.CASES["fused_t2"]
    ent = lg.umbrella_entries(fz.n2)
    differ = 0
    for t, s, e in fz.ranges:
        lo, ub, hp = lg.window(ent, s, e, False)
        _, ub_t, ht = lg.window(ent, s, e, True)
        if lg.is_wide(lo, ub) and lg.is_wide(lo, ub_t) and set(hp) - set(ht) and all(ent[i][0] == ent[i][1] for i in set(hp) - set(ht)):
            differ += 1
    assert len(fz.ranges) >= 160 and differ >= 20
