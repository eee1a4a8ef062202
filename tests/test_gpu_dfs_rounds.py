"""The batch engine's DFS rounds (Engine::run_dfs: dfs_pop_select / flags / scatter, the hop, the update, frontier_to_stack, the
two radix sorts, run_heads / run_starts, dfs_merge_kernel, dfs_compact_kernel) and the folding of its visited tables
(Engine::compact_tables), on the fixtures of tests/dfs_gen.py -- which tests/test_dfs_gen_cpu.py holds to the oracle and to
their edges.  Every check is exact equality; no case is skipped or sampled.

For every fixture and every parameter set it is meant for, with walk_kernel = 0 (the batch engine):
  rows        query_batch's equal the oracle's, in order (`projected` too)
  stats       query_batch_stats' counts are the rows minus the self row; stats.levels is the model's most explored pops
  counters    "dfs_rounds" and "visited_compactions" rise by the model's rounds and folds, on either call; "walk_launches" stays
  the walk    (plain DFS) under walk_kernel = 1 the same rows, counts and checksums; "walk_launches" rises, "walk_fallbacks" and
              "dfs_rounds" do not
MultiImpg fixtures run their DFS and BFS worklists against the oracle built from the same files.  The masked start is checked
against the oracle alone (the walk declines it).  Further legs: store_cigar (kept levels), chunk_ranges = 7, a plain BFS that
folds (Engine::run), and a sharded index (devices [0, 0, 0], lanes 2) whose ranks keep counters of their own.

Logic-only mutations of the kernels, each built beside the tree and run on an MI355X against this file, never kept (none can
index out of bounds: each changes a comparison or a value, no address).  What failed:
  dfs_merge_kernel keeps min of the depths        depth-merge, merge-three, around, store_cigar[depth-merge, max_depth 3]
  `we > rs` for `we >= rs` in dfs_merge_kernel    depth-merge, its mirror, merge-three, around, deep-between-* (3), masked-start,
                                                  store_cigar[depth-merge] (2)
  dfs_pop_select_kernel ignores the depth test    27 of 39: every fixture run under a depth limit that its walk reaches
  compact_last_kernel flags the first of a key    ladder-back-1, ladder-back-300, store_cigar[ladder-back-1], both BFS folds of
                                                  ladder-back.  ladder-1 and ladder-300 pass under it: no hit of the plain ladder
                                                  lands on a range visited before, so an old list changes nothing there.  (A
                                                  first form of ladder-back, with ways back into the ladder, did not end under
                                                  this mutation -- the walk climbs, folds, forgets and is sent back: a test
                                                  must fail, not spin, hence the dead-end side branch and dfs_gen's rule that
                                                  every fixture is a graph without cycles.)
"""
import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import dfs_gen as dg

pytestmark = pytest.mark.gpu
COUNTERS = ("dfs_rounds", "visited_compactions", "walk_launches", "walk_fallbacks")
_model = {}


def modelled(case, kw):
    key = (case.name, tuple(sorted(kw.items())))
    if key not in _model:
        _model[key] = dg.run(dg.Index(case.texts), case.queries, kw)[1]
    return _model[key]


def both(tmp_path, texts, **how):
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ("f%d.paf" % i)))
        with open(paths[-1], "w") as f:
            f.write(t)
    g = impg_amd.GpuImpg.from_paf(paths if len(paths) > 1 else paths[0], bidirectional=False, **how)
    c = o.OracleIndex(paf_paths=paths, bidirectional=False, preparse=True)
    assert [g.seq_name(i) for i in range(g.num_seqs())] == [c.seq_name(i) for i in range(c.num_seqs())]
    return g, c


def ctr(g):
    return {k: g.counter(k) for k in COUNTERS}


def moved(g, before):
    after = ctr(g)
    return {k: after[k] - before[k] for k in COUNTERS}


def ranges_of(g, queries):
    return [(g.seq_id(t), s, e) for t, s, e in queries]


def oracle_rows(c, ranges, mask, kw):
    rows, proj = [], 0
    for t, s, e in ranges:
        rows.append(c.query(t, s, e, masked_regions=mask, **kw))
        proj += c.last_projection_count()
    return rows, proj


def same_rows(res, want, proj, what):
    for i, w in enumerate(want):
        assert res[i].tolist() == w.tolist(), (what, i)
    assert res.projected == proj, what


def batch_engine(g, c, case, kw, rounds, folds, levels):
    """the walk_kernel = 0 leg: rows, stats and the counters of both calls"""
    ranges = ranges_of(g, case.queries)
    want, proj = oracle_rows(c, ranges, None, kw)
    g.set_option("walk_kernel", 0)
    before = ctr(g)
    res = g.query_batch(ranges, impg_amd.make_params(**kw))
    d = moved(g, before)
    same_rows(res, want, proj, (case.name, kw))
    assert d == dict(dfs_rounds=rounds, visited_compactions=folds, walk_launches=0, walk_fallbacks=0), (case.name, kw, d)
    before = ctr(g)
    st, cnt, ck = g.query_batch_stats(ranges, impg_amd.make_params(**kw))
    d = moved(g, before)
    assert cnt.tolist() == [len(w) - 1 for w in want], (case.name, kw)  # (a range's own row is not a hit)
    assert st.projected == proj and st.levels == levels, (case.name, kw, st.levels, levels)
    assert d == dict(dfs_rounds=rounds, visited_compactions=folds, walk_launches=0, walk_fallbacks=0), (case.name, kw, d)
    return ranges, want, proj, cnt, ck


def the_walk(g, case, kw, ranges, want, proj, cnt, ck):
    """the walk_kernel = 1 leg of a plain DFS: the same answers, by the walk"""
    g.set_option("walk_kernel", 1)
    before = ctr(g)
    st, cnt1, ck1 = g.query_batch_stats(ranges, impg_amd.make_params(**kw))
    d = moved(g, before)
    assert d["walk_launches"] > 0 and (d["walk_fallbacks"], d["dfs_rounds"], d["visited_compactions"]) == (0, 0, 0), (case.name, kw, d)
    assert (cnt1.tolist(), ck1.tolist(), st.projected) == (cnt.tolist(), ck.tolist(), proj), (case.name, kw)
    before = ctr(g)
    res = g.query_batch(ranges, impg_amd.make_params(**kw))
    d = moved(g, before)
    assert d["walk_launches"] > 0 and (d["walk_fallbacks"], d["dfs_rounds"]) == (0, 0), (case.name, kw, d)
    same_rows(res, want, proj, (case.name, kw, "walk"))
    g.set_option("walk_kernel", 0)


@pytest.mark.parametrize("name", [n for n, c in dg.CASES.items() if c.modelled])
def test_fixture(tmp_path, name):
    case = dg.CASES[name]
    g, c = both(tmp_path, case.texts)
    for kw in case.kws:
        bt = modelled(case, kw)
        got = batch_engine(g, c, case, kw, bt.rounds, bt.folds, bt.levels)
        if not case.multi:
            the_walk(g, case, kw, *got)
        else:  # the worklist of either end answers whatever the fixture was built for
            other = dict(kw, dfs=not kw["dfs"])
            bo = dg.run(dg.Index(case.texts), case.queries, other)[1]
            batch_engine(g, c, case, other, bo.rounds, bo.folds, bo.levels)


def test_ladder_counters_are_the_issues():
    """the single-query ladder as numbers: 2 folds; 121 rounds, not the issue's 120 -- that is the count of its projections (and of
    its tables): the 121st record, A:[60000, +100), is popped and looked up like the others, and finds nothing"""
    bt = modelled(dg.CASES["ladder-1"], dg.D(0))
    assert (bt.rounds, bt.levels, bt.folds) == (121, 121, 2) and sum(1 for k in bt.queries[0].keys if k) == 120


def test_multi_step_plain_order(tmp_path):
    """the step itself, not transitive: sort5_kernel's order over 63 .. 129 slots is the oracle's, ties and self copies included"""
    for h in dg.STEP_HITS:
        case = dg.CASES["multi-step-%d" % h]
        sub = tmp_path / str(h)
        sub.mkdir()
        g, c = both(sub, case.texts)
        ranges = ranges_of(g, case.queries)
        want, proj = oracle_rows(c, ranges, None, dict(multi_impg=True))
        same_rows(g.query_batch(ranges, impg_amd.make_params(multi_impg=True)), want, proj, h)
        assert len(want[0]) == h - 1


def test_masked_start(tmp_path):
    """first pieces that touch (a mask with empty ranges inside the queried range): the first round pushes nothing and must merge
    them all the same.  The walk declines the batch.  Rounds by hand: T:[60, 100), T:[0, 60), Y, then Z (no limit) or a round
    that only drops Z (max_depth 2): 4 either way."""
    case = dg.CASES["masked-start"]
    g, c = both(tmp_path, case.texts)
    ranges = ranges_of(g, case.queries)
    mask = {q: (c.seq_len(q), case.mask.get(c.seq_name(q), [])) for q in range(c.num_seqs())}
    for kw in case.kws:
        want, proj = oracle_rows(c, ranges, mask, kw)
        assert len(want[0]) == 5 and want[0]["q_last"].tolist()[3] == 60
        for walk_kernel in (0, 1):
            g.set_option("walk_kernel", walk_kernel)
            before = ctr(g)
            res = g.query_batch(ranges, impg_amd.make_params(**kw), masked_regions=mask)
            d = moved(g, before)
            same_rows(res, want, proj, (kw, walk_kernel))
            assert d == dict(dfs_rounds=4, visited_compactions=0, walk_launches=0, walk_fallbacks=0), (kw, walk_kernel, d)


@pytest.mark.parametrize("name,kw", [("depth-merge", dg.D(3)), ("depth-merge", dg.D(4)), ("ladder-back-1", dg.D(0)), ("long-run", dg.D(2))])
def test_store_cigar(tmp_path, name, kw):
    """store_cigar keeps every round's level: rows and CIGARs equal the oracle's, the rounds and folds are the model's"""
    case = dg.CASES[name]
    g, c = both(tmp_path, case.texts)
    bt = modelled(case, kw)
    ranges = ranges_of(g, case.queries)
    before = ctr(g)
    res = g.query_batch(ranges, impg_amd.make_params(store_cigar=True, **kw))
    d = moved(g, before)
    for i, (t, s, e) in enumerate(ranges):
        want, wcg = c.query_cigar(t, s, e, **kw)
        assert res[i].tolist() == want.tolist(), (name, i)
        assert [x.tolist() for x in res.cigars(i)] == [x.tolist() for x in wcg], (name, i)
    assert d == dict(dfs_rounds=bt.rounds, visited_compactions=bt.folds, walk_launches=0, walk_fallbacks=0), (name, d)


def test_chunked_batch(tmp_path):
    """chunk_ranges = 7: 43 chunks of the 300-query ladder, each a run_dfs of its own; rows only"""
    case = dg.CASES["ladder-300"]
    g, c = both(tmp_path, case.texts)
    g.set_option("walk_kernel", 0)
    g.set_option("chunk_ranges", 7)
    ranges = ranges_of(g, case.queries)
    for kw in (dg.D(7), dg.D(2)):
        want, proj = oracle_rows(c, ranges, None, kw)
        same_rows(g.query_batch(ranges, impg_amd.make_params(**kw)), want, proj, kw)


@pytest.mark.parametrize("name", ["ladder-1", "ladder-300", "ladder-back-1", "ladder-back-300"])
def test_plain_bfs_folds(tmp_path, name):
    """Engine::run's levels fold the same tables: on the ladder every level of a query is one range, the record its DFS pops in
    that round -- the model's folds hold (where a query is one chain), and no DFS round is counted."""
    case = dg.CASES[name]
    g, c = both(tmp_path, case.texts)
    g.set_option("walk_kernel", 0)
    bt = modelled(case, dg.D(0))
    ranges = ranges_of(g, case.queries)
    want, proj = oracle_rows(c, ranges, None, dg.B(0))
    before = ctr(g)
    res = g.query_batch(ranges, impg_amd.make_params(**dg.B(0)))
    d = moved(g, before)
    same_rows(res, want, proj, name)
    chains = all(t.peak == 1 for t in bt.queries)  # (ladder-back: the side branch is a second record on the stack, a second range of a level)
    assert chains == ("back" not in name) and bt.folds >= 2
    assert d == dict(dfs_rounds=0, visited_compactions=bt.folds if chains else d["visited_compactions"], walk_launches=0, walk_fallbacks=0), d
    assert d["visited_compactions"] >= 2


def test_sharded(tmp_path):
    """the 300-query ladder and the too-deep fixture on three ranks of one device: queries die in different rounds on different
    ranks (a rank whose stacks are empty still takes part in every hop).  Rows against the oracle; the front handle counts nothing."""
    text = dg.CASES["too-deep-back"].texts[0] + dg.CASES["ladder-300"].texts[0]
    g, c = both(tmp_path, [text], devices=[0, 0, 0], lanes=2)
    queries = dg.ladder_queries()
    queries[40:40] = dg.TOO_DEEP_QUERIES
    ranges = ranges_of(g, queries)
    for kw in (dg.D(2), dg.D(0)):
        want, proj = oracle_rows(c, ranges, None, kw)
        same_rows(g.query_batch(ranges, impg_amd.make_params(**kw)), want, proj, kw)
        st, cnt, ck = g.query_batch_stats(ranges, impg_amd.make_params(**kw))
        assert cnt.tolist() == [len(w) - 1 for w in want], kw
    assert len({len(w) for w in want}) > 100 and np.all(cnt[40:43] > 0)
