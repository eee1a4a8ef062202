"""tests/dfs_gen.py checked without a GPU: its model agrees with the oracle on every fixture it covers, its fold threshold is the
source's, and every fixture reaches the edge it was built for -- so tests/test_gpu_dfs_rounds.py cannot silently stop sitting
on one.  The discriminating answers are written out as literals."""
import os
import re
from collections import Counter

import pytest

from oracle import oracle as o
from tests import dfs_gen as dg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "impg_amd", "csrc")
_memo = {}


def src(name):
    return open(os.path.join(CSRC, name)).read()


def oracle_index(case, tmp_path):
    if len(case.texts) == 1:
        return o.OracleIndex(paf_text=case.texts[0], bidirectional=False, preparse=True)
    paths = []
    for i, t in enumerate(case.texts):
        paths.append(str(tmp_path / ("f%d.paf" % i)))
        with open(paths[-1], "w") as f:
            f.write(t)
    return o.OracleIndex(paf_paths=paths, bidirectional=False, preparse=True)


def modelled(name, kw):
    """the model's (rows, trace) of a case under one parameter set, computed once"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _memo:
        case = dg.CASES[name]
        _memo[key] = dg.run(dg.Index(case.texts), case.queries, kw)
    return _memo[key]


def named(ix, rows):
    """rows as (name, first, last) of their query side"""
    return [(ix.names[r[0]], r[1], r[2]) for r in rows]


def test_fold_threshold_is_the_sources():
    assert re.findall(r"constexpr int MAX_VISITED_TABLES = (\d+);", src("kernels.hpp")) == [str(dg.MAX_VISITED_TABLES)]
    e = src("engine.cpp")
    assert e.count("if (tables.size() + %d >= (size_t)MAX_VISITED_TABLES) compact_tables();" % dg.FOLD_SLACK) == 1
    assert len(re.findall(r"[^:]compact_tables\(\);", e)) == 1  # the one place that folds
    k = src("kernels.hip")
    # the comparisons the fixtures sit on, as the kernels write them (a mutation of one of them must fail a GPU case, see there)
    for text in ("if (we >= rs) {", "we = max(we, re);  // merged element keeps the first one's depth",
                 "if (max_depth > 0 && depth[i] >= max_depth) return;", "flag[i] = (i + 1 == n || skeys[i + 1] != skeys[i]) ? 1u : 0u;",
                 "keep_flag[i] = have && (pop_front ? i > x : i < x) ? 1u : 0u;"):
        assert k.count(text) == 1, text
    assert "__launch_bounds__(64) void dfs_merge_kernel" in k and "dfs_merge_kernel<<<cdiv(n_groups, 64), 64, 0, s>>>" in k


@pytest.mark.parametrize("name", [n for n, c in dg.CASES.items() if c.modelled])
def test_model_agrees_with_the_oracle(tmp_path, name):
    case = dg.CASES[name]
    c = oracle_index(case, tmp_path)
    ix = dg.Index(case.texts)
    assert ix.names == [c.seq_name(i) for i in range(c.num_seqs())]
    for kw in case.kws:
        rows, bt = modelled(name, kw)
        for q, (t, s, e) in enumerate(case.queries):
            want = c.query(c.seq_id(t), s, e, **kw)
            assert Counter(rows[q]) == Counter(map(tuple, want.tolist())), (name, kw, q)
            assert case.multi or c.last_projection_count() == len(want) - 1  # (MultiImpg projects the hits it then skips, too)
        assert all(t.overlaps == 0 for t in bt.queries), name  # records of one sequence touch, never overlap (dfs_gen's docstring)


def test_masked_start_against_the_oracle():
    """the one fixture the model does not cover: its first pieces touch and are merged by the first re-sort, pushes or not"""
    case = dg.CASES["masked-start"]
    c = oracle_index(case, None)
    mask = {q: (c.seq_len(q), case.mask.get(c.seq_name(q), [])) for q in range(c.num_seqs())}
    T, Y, Z = c.seq_id("T"), c.seq_id("Y"), c.seq_id("Z")
    rows = c.query(T, 0, 100, masked_regions=mask, **dg.D(0)).tolist()
    assert rows == [(T, 0, 30, T, 0, 30), (T, 30, 60, T, 30, 60), (T, 60, 100, T, 60, 100), (Y, 0, 60, T, 0, 60), (Z, 0, 60, Y, 0, 60)]


def where(ix, rows, name):
    return sorted((a, b) for n, a, b in named(ix, rows) if n == name)


def test_depth_merge_literals():
    """no W row at depth 3, a W row at depth 4 and without a limit; the mirror's W:0-200 at depth 3"""
    ix = dg.Index(dg.CASES["depth-merge"].texts)
    assert ix.names == dg.MERGE_ORDER
    for depth, w in ((3, []), (4, [(0, 200)]), (0, [(0, 200)])):
        rows, bt = modelled("depth-merge", dg.D(depth))
        assert where(ix, rows[0], "W") == w, depth
        assert sorted(r for r in named(ix, rows[0]) if r[0] != "W") == [("T", 0, 100), ("X", 0, 100), ("X", 100, 200), ("Y", 0, 100), ("Z", 0, 100)]
        t = bt.queries[0]
        assert (t.first_deeper, t.second_deeper, t.equal_depth) == (1, 0, 0)  # X:[0, 100) of depth 3 in front of X:[100, 200) of depth 1
        assert (t.explored, t.dropped, t.rounds) == ((3, 1, 4) if depth == 3 else (4, 1, 5) if depth == 4 else (5, 0, 5))
    for depth in (3, 4):
        rows, bt = modelled("depth-merge-mirror", dg.D(depth))
        assert where(ix, rows[0], "W") == [(0, 200)], depth  # the merged record keeps depth 1: explored, its deep half included
        t = bt.queries[0]
        assert (t.first_deeper, t.second_deeper, t.equal_depth) == (0, 1, 0)
    for name, span in (("merge-three", 300), ("around", 100)):
        for depth, w in ((3, []), (4, [(0, span)])):
            rows, bt = modelled(name, dg.D(depth))
            assert where(ix, rows[0], "W") == w, (name, depth)
            t = bt.queries[0]
            # deep - shallow - deep: the first merge has the deeper record in front, the second (depth 3 kept) again
            assert (t.first_deeper, t.second_deeper, t.equal_depth) == (1, 0, 1) and t.longest_run == 3, name
    merges = [modelled(n, dg.D(3))[1].queries[0] for n in ("depth-merge", "depth-merge-mirror", "merge-three", "around")]
    assert sum(t.first_deeper for t in merges) >= 1 and sum(t.second_deeper for t in merges) >= 1 and sum(t.equal_depth for t in merges) >= 1


@pytest.mark.parametrize("name,kw", [("too-deep-back", dg.D(2)), ("too-deep-back-multi", dg.multi([dg.D(2)])[0]),
                                     ("too-deep-front-multi", dg.multi([dg.B(2)])[0])])
def test_too_deep_ends(name, kw):
    """at least 2 drops behind an explored pop and one whole-run drop, while another query lives on"""
    rows, bt = modelled(name, kw)
    p, c, s = bt.queries
    assert (p.explored, p.dropped, p.drops_behind, p.whole_run_drops, p.rounds) == (3, 3, 2, 1, 4)
    assert (c.explored, c.dropped, c.drops_behind, c.whole_run_drops, c.rounds) == (7, 6, 1, 1, 8)
    assert (s.explored, s.dropped, s.whole_run_drops, s.rounds) == (2, 0, 0, 2)
    assert bt.rounds == 8 and bt.levels == 7 and bt.rounds > p.rounds  # P dies in a round that only drops; C lives on
    ix = dg.Index(dg.CASES[name].texts)
    assert sorted(n for n, _, _ in named(ix, rows[0])) == ["L", "M", "P", "R", "U1", "U2"]


@pytest.mark.parametrize("name,kw", [("deep-between-back", dg.D(3)), ("deep-between-back-multi", dg.multi([dg.D(3)])[0]),
                                     ("deep-between-front-multi", dg.multi([dg.B(3)])[0])])
def test_deep_between(name, kw):
    """a too-deep record between two explorable ones stays: W:0-200, not W:0-100"""
    rows, bt = modelled(name, kw)
    t = bt.queries[0]
    ix = dg.Index(dg.CASES[name].texts)
    assert where(ix, rows[0], "W") == [(0, 200)]
    assert t.deep_kept >= 1 and t.second_deeper == 1 and t.drops_behind == 1 and t.whole_run_drops == 0
    assert (t.explored, t.dropped, t.rounds) == (7, 1, 7)  # T, F, G, E2, X, E1 (behind W, dropped), V


@pytest.mark.parametrize("n", dg.COMB_N)
def test_comb(n):
    """a peak stack equal to N, in N groups; then N (max_depth 2) or 2 N (no limit) more rounds through the folds"""
    name = "comb-%d" % n
    rows, bt = modelled(name, dg.D(2))
    t = bt.queries[0]
    assert t.peak == n and t.sizes[1] == n and t.longest_run == 1
    assert (t.explored, t.dropped, t.drops_behind, t.whole_run_drops, t.rounds) == (1 + n, n, 1, 1, 2 + n)
    assert len(rows[0]) == 1 + 2 * n
    assert bt.folds == n // (dg.MAX_VISITED_TABLES - dg.FOLD_SLACK - 1) and bt.folds >= 1
    rows, bt = modelled(name, dg.D(0))
    t = bt.queries[0]
    assert (t.explored, t.dropped, t.rounds, t.peak) == (1 + 2 * n, 0, 1 + 2 * n, n) and len(rows[0]) == 1 + 2 * n
    assert bt.levels == 1 + 2 * n and bt.folds == n // (dg.MAX_VISITED_TABLES - dg.FOLD_SLACK - 1)


def test_long_run():
    rows, bt = modelled("long-run", dg.D(2))
    t, u = bt.queries
    touching = sum(1 for i in range(dg.LONG_RUN - 1) if i % 5 == 2)
    assert t.longest_run == dg.LONG_RUN and t.equal_depth == touching and touching == 60 and t.peak == dg.LONG_RUN - touching
    assert u.longest_run == 1 and u.peak == 1
    ix = dg.Index(dg.CASES["long-run"].texts)
    w = where(ix, rows[0], "W")
    assert len(w) == dg.LONG_RUN - touching and sorted(b - a for a, b in w)[-1] == 200 and sum(b - a for a, b in w) == 100 * dg.LONG_RUN
    assert bt.rounds == 1 + (dg.LONG_RUN - touching) + 1 and bt.flat[1] == dg.LONG_RUN - touching + 1


def test_ladder():
    """The single query explores 121 records -- the issue's count of 120 is that of its projections: the last record, A:[60000,
    +100), is explored like the others and finds nothing -- and makes 120 tables: two folds, and before the first the key
    (0, A) lies in 23 tables.  The batch's queries end in different rounds while the flat stack crosses 256."""
    rows, bt = modelled("ladder-1", dg.D(0))
    t = bt.queries[0]
    assert (t.explored, t.rounds, t.dropped, t.peak) == (121, 121, 0, 1) and len(rows[0]) == 121
    assert sum(1 for k in t.keys if k) == 120 and t.explored >= 120
    assert bt.folds == 2 and bt.first_fold_key_tables >= 23 and bt.first_fold_key_tables == 23
    rows, bt = modelled("ladder-1", dg.D(7))
    assert (bt.queries[0].explored, bt.queries[0].dropped, bt.rounds, bt.folds) == (7, 1, 8, 0) and len(rows[0]) == 8
    rows, bt = modelled("ladder-300", dg.D(0))
    ends = {t.rounds for t in bt.queries}
    assert len(ends) >= 100 and bt.rounds == max(ends) and min(ends) < 10 and bt.folds >= 2
    assert bt.flat[0] == 300 and min(bt.flat) < 256 < max(bt.flat) and any(a > 256 >= b for a, b in zip(bt.flat, bt.flat[1:]))
    assert bt.first_fold_key_tables >= 23


def test_ladder_back():
    """the key (0, S) lies in two tables when the first fold comes, the list that knows S:[200, 300) is the newer one, and the
    range is hit again after the folds; S:[400, 500) is visited between the folds and hit again after the second"""
    rows, bt = modelled("ladder-back-1", dg.D(0))
    t = bt.queries[0]
    ix = dg.Index(dg.CASES["ladder-back-1"].texts)
    assert (t.explored, t.rounds, len(rows[0]), bt.folds) == (126, 126, 128, 2)
    assert where(ix, rows[0], "Z") == [(0, 100), (200, 300)]  # once each
    assert where(ix, rows[0], "S") == [(0, 100), (200, 300), (200, 300), (400, 500), (400, 500)]
    keyed = [k for k, keys in enumerate(t.keys) if keys]          # the pops that made a table
    per_fold = dg.MAX_VISITED_TABLES - dg.FOLD_SLACK - 1          # tables a fold away from the last one
    fold1, fold2 = keyed[per_fold - 1], keyed[2 * per_fold - 1]   # the pops whose table brought a fold
    on_s = [k for k, keys in enumerate(t.keys) if ix.ids["S"] in keys]
    assert len(on_s) == 5 and on_s[0] < on_s[1] < fold1 < on_s[2] < fold2 < on_s[3] < on_s[4]
    rows, bt = modelled("ladder-back-300", dg.D(0))
    assert bt.folds >= 2


@pytest.mark.parametrize("h", dg.STEP_HITS)
def test_multi_step(tmp_path, h):
    """exactly h slots in the first step (the self copies and the ties among them), over three files"""
    case = dg.CASES["multi-step-%d" % h]
    lines = [line for t in case.texts for line in t.splitlines() if line.split("\t")[5] == "T" and int(line.split("\t")[7]) < dg.FAR]
    assert len(lines) == h and len(set(lines)) < h - 1  # (two self copies, and ties besides)
    per_file = [sum(1 for line in t.splitlines() if line.split("\t")[5] == "T" and int(line.split("\t")[7]) < dg.FAR) for t in case.texts]
    assert len(per_file) == 3 and min(per_file) > 0
    c = oracle_index(case, tmp_path)
    T = c.seq_id("T")
    plain = c.query(T, 1000, 1500, multi_impg=True)
    assert len(plain) == 1 + h - 2  # the self row once, every other hit
    assert c.last_projection_count() == h
