"""Every tier of the visited update at its capacity edges, against the oracle -- and proof that each one ran.

big_groups_kernel hands a (query, sequence) group to one of five kernels by cap = old list length + hits of the level; the
wave kernels replay in place on the global slice once a list outgrows (or never fits) their LDS buffer and sort more
pieces than it holds tile by tile; the lane kernels move a group's pieces out of the LDS column when they meet its list.
tests/update_gen.py builds one PAF per edge and says, from a plain model, what level 1 of it reaches; here each case runs
on the batch engine (walk_kernel 0) with update_stats 1, rows against the oracle, and the update_* counters of a run with
exactly one update (max_depth 2) must show exactly the groups and paths the model names -- so a case that lands on another
tier, or a counter that stops counting, fails instead of passing on the wrong path."""
import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import update_gen as ug

pytestmark = pytest.mark.gpu

TIER_COUNTER = dict(lane="update_lane_groups", mid="update_mid_groups", tiny="update_wave_tiny_groups",
                    small="update_wave_small_groups", large="update_wave_large_groups")
PATH_COUNTER = dict(inplace="update_inplace_groups", tiled="update_tiled_sort_groups", spill="update_lane_spill_groups")
COUNTERS = list(TIER_COUNTER.values()) + list(PATH_COUNTER.values())


@pytest.fixture(scope="module", autouse=True)
def sorted_visits():
    o.set_sorted_visits(True)  # (with ORDER_SORTED below: a level's hits in the order the cases are written in)
    yield
    o.set_sorted_visits(False)


def snapshot(g):
    return {k: g.counter(k) for k in COUNTERS}


def same_rows(g, case, ranges, want, masked, **kw):
    """query_batch against the oracle's rows of the distinct ranges (the batch repeats them case.reps times)."""
    res = g.query_batch(ranges, impg_amd.make_params(**case.kw(**kw)), masked_regions=masked)
    rows, proj = want
    lens = np.array([len(r) for r in rows] * case.reps, dtype=np.uint64)
    assert np.array_equal(np.asarray(res.offsets), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)), (case.name, kw)
    assert res.intervals.tolist() == np.concatenate(rows * case.reps).tolist(), (case.name, kw)
    assert res.projected == proj * case.reps, (case.name, kw)


@pytest.mark.parametrize("name", list(ug.CASES))
def test_update_tier(tmp_path, name):
    case = ug.CASES[name]
    text, named = case.paf()
    path = str(tmp_path / "u.paf")
    with open(path, "w") as f:
        f.write(text)
    g = impg_amd.GpuImpg.from_paf(path, bidirectional=False, order=impg_amd.ORDER_SORTED)
    c = o.OracleIndex(paf_paths=[path], bidirectional=False, preparse=True)
    assert [g.seq_name(i) for i in range(g.num_seqs())] == [c.seq_name(i) for i in range(c.num_seqs())]
    g.set_option("walk_kernel", 0)  # (the per-query walk has an update of its own: every run here is the batch engine's)
    g.set_option("update_stats", 1)
    ranges = [(g.seq_id(t), s, e) for t, s, e in named]
    distinct = ranges[:len(ranges) // case.reps]
    masked = case.masked(g.seq_id) if case.mask else None
    many = case.reps > 1
    runs = [(dict(max_depth=2), masked), (dict(max_depth=4), masked)]
    if not many:  # (one batch of 10^4..10^5 queries is what those cases are about: twice is enough)
        runs += [(dict(dfs=True, max_depth=3), masked)]
        if masked is not None:
            runs += [(dict(max_depth=4), None), (dict(dfs=True, max_depth=3), None)]
    want = []
    for kw, m in runs:
        rows, proj = [], 0
        for t, s, e in distinct:
            rows.append(c.query(t, s, e, masked_regions=m, **case.kw(**kw)))
            proj += c.last_projection_count()
        want.append((rows, proj))
    assert sum(len(r) for r in want[1][0]) > len(case.hits)
    deep = None
    if not many:
        # The three updates of the max_depth 4 run: level 1 as the model says; level 2 is R's group (no old list, as many
        # hits as the oracle's max_depth 3 rows from Q to R); level 3 is Q's group again: the list level 1 left -- its
        # LENGTH from the model -- plus as many hits as the oracle's rows from R to Q.  A replay that leaves a list of the
        # right coverage but the wrong length (touching ranges not merged) changes no row; it changes this tier.
        t, s, e = distinct[0]
        r3 = c.query(t, s, e, masked_regions=masked, **case.kw(max_depth=3))
        R, Q = g.seq_id("R"), g.seq_id("Q")
        h2 = int(((r3["target_id"] == Q) & (r3["query_id"] == R)).sum())
        h3 = int(((r3["target_id"] == R) & (r3["query_id"] == Q)).sum())
        m0 = case.model(False)
        deep = [m0["tier"]] + ([ug.tier_of(h2, 0)] if h2 else []) + ([ug.tier_of(m0["final_len"] + h3, m0["final_len"])] if h3 else [])
    stats = []
    for f in (0, 1):
        g.set_option("filter_covered", f)
        # one update, one group per query: the counters say exactly which kernel took it and what it reached
        before = snapshot(g)
        same_rows(g, case, ranges, want[0], masked, **runs[0][0])
        after = snapshot(g)
        got = {k: after[k] - before[k] for k in COUNTERS}
        exp = dict.fromkeys(COUNTERS, 0)
        if many:
            exp[TIER_COUNTER[case.expect["tier"]]] = len(ranges)  # (isolated hits: the pre-pass drops none)
        else:
            m = case.model(bool(f))
            exp[TIER_COUNTER[m["tier"]]] = 1
            for k, key in PATH_COUNTER.items():
                exp[key] = int(bool(m[k]))
        assert got == exp, (name, f, None if many else m)
        for (kw, mk), w in list(zip(runs, want))[1:]:
            before = snapshot(g)
            same_rows(g, case, ranges, w, mk, **kw)
            if deep is not None and f == 0 and (kw, mk) == runs[1]:  # (the pre-pass off: every hit counts towards cap)
                after = snapshot(g)
                got = {k: after[k] - before[k] for k in TIER_COUNTER.values()}
                assert got == {key: deep.count(tier) for tier, key in TIER_COUNTER.items()}, (name, deep)
        # (query_batch_stats takes no mask: level 1 finds no old list here, so this compares the pre-pass on the lists of
        # levels 2 and 3 only -- the masked row comparisons above are what runs both settings on the case's own boundary)
        st, cnt, ck = g.query_batch_stats(ranges, impg_amd.make_params(**case.kw(max_depth=4)))
        stats.append((int(st.projected), cnt.tolist(), ck.tolist()))
    assert stats[0] == stats[1], name  # the same counts and checksums with and without the pre-pass
    g.set_option("filter_covered", 0)


def test_update_stats_off_counts_nothing(tmp_path):
    """Without the option a query leaves every update_* counter where it was."""
    case = ug.CASES["grow1153"]
    text, named = case.paf()
    path = str(tmp_path / "u.paf")
    with open(path, "w") as f:
        f.write(text)
    g = impg_amd.GpuImpg.from_paf(path, bidirectional=False, order=impg_amd.ORDER_SORTED)
    g.set_option("walk_kernel", 0)
    ranges = [(g.seq_id(t), s, e) for t, s, e in named]
    g.query_batch(ranges, impg_amd.make_params(**case.kw(max_depth=3)))
    assert snapshot(g) == dict.fromkeys(COUNTERS, 0)
    g.set_option("update_stats", 1)
    g.query_batch(ranges, impg_amd.make_params(**case.kw(max_depth=3)))
    s = snapshot(g)
    assert s["update_inplace_groups"] == 1 and s["update_tiled_sort_groups"] == 1 and s["update_wave_small_groups"] >= 1
