"""The per-query walk's MultiImpg arm (walk_device.inc, walk_body<.., MULTI>; Engine::walk_applicable / run_walk; walk_two_pass): a
MultiImpg worklist, popped at either end, answered by the walk kernel.  Every check is exact equality against the oracle built
from the same files; no case is skipped or sampled.

Under walk_kernel = 1, for every call:
  rows      query_batch's equal the oracle's, in order, `projected` too
  stats     query_batch_stats' counts, checksums and `projected` equal the same call under walk_kernel = 0 (the batch engine)
  counters  walk_launches rose, walk_fallbacks and dfs_rounds did not, walk_overflow == 0
(query_batch_stats takes no subset filter and no mask: those parameter sets leave it out.)

  1  the MultiImpg fixtures of tests/dfs_gen.py and every fixture of tests/multi_walk_gen.py, every parameter set, both ends
  2  dfs_gen's 300-query ladder as one file: more queries than a launch has workgroups to start with, dealt from the shared counter
  3  a random index with cycles, both strands and indels: 128 ranges as one batch and one by one
  4  a pop of 4 097 pairs (cause bit 2) and a stack pool of 65 544 records (bit 32) fall back, their twins of 4 096 / 65 528 stay;
     after a fallback the next MultiImpg query is the walk's again.  (The pop budget, bit 256, is not provoked: its constant is
     held to the source by tests/test_multi_walk_gen_cpu.py.)
  5  store_cigar, a mask and a sharded handle are still declined: walk_launches does not move, the rows are the oracle's
"""
import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import dfs_gen as dg
from tests import multi_walk_gen as mg
from tests import walk_gen as wg

pytestmark = pytest.mark.gpu
COUNTERS = ("walk_launches", "walk_fallbacks", "walk_overflow", "dfs_rounds")
ENDS = (True, False)  # dfs: popped at the back, at the front


def both(tmp_path, texts, bidirectional=False, **how):
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ("f%d.paf" % i)))
        with open(paths[-1], "w") as f:
            f.write(t)
    g = impg_amd.GpuImpg.from_paf(paths if len(paths) > 1 else paths[0], bidirectional=bidirectional, **how)
    c = o.OracleIndex(paf_paths=paths, bidirectional=bidirectional, preparse=True)
    assert [g.seq_name(i) for i in range(g.num_seqs())] == [c.seq_name(i) for i in range(c.num_seqs())]
    return g, c


def ctr(g):
    return {k: g.counter(k) for k in COUNTERS}


def walked(g, before, what):
    after = ctr(g)
    assert after["walk_launches"] > before["walk_launches"], (what, before, after)
    assert (after["walk_fallbacks"], after["dfs_rounds"]) == (before["walk_fallbacks"], before["dfs_rounds"]) and after["walk_overflow"] == 0, (what, before, after)


def declined(g, before, what):
    after = ctr(g)
    assert (after["walk_launches"], after["walk_fallbacks"]) == (before["walk_launches"], before["walk_fallbacks"]), (what, before, after)


def fell(g, before, bit, what):
    after = ctr(g)
    assert after["walk_fallbacks"] > before["walk_fallbacks"] and after["walk_launches"] == before["walk_launches"], (what, before, after)
    assert after["walk_overflow"] & bit and not after["walk_overflow"] & ~bit & (wg.NEVER | 256), (what, hex(after["walk_overflow"]))


def keep_of(c, names):
    return None if names is None else np.array([c.seq_name(i) in names for i in range(c.num_seqs())], dtype=np.uint8)


def oracle_rows(c, ranges, kw, keep=None, mask=None):
    rows, proj = [], 0
    for t, s, e in ranges:
        rows.append(c.query(t, s, e, subset_keep=keep, masked_regions=mask, **kw))
        proj += c.last_projection_count()
    return rows, proj


def same_rows(res, want, proj, what):
    for i, w in enumerate(want):
        assert res[i].tolist() == w.tolist(), (what, i)
    assert res.projected == proj, what


def by_the_walk(g, c, ranges, kw, keep=None, what=None, want=None):
    """one parameter set at one end: the rows by the walk against the oracle; the stats by the walk against the batch engine's"""
    g.set_option("walk_kernel", 1)
    if want is None:
        want = oracle_rows(c, ranges, kw, keep)
    before = ctr(g)
    res = g.query_batch(ranges, impg_amd.make_params(**kw), subset_keep=keep)
    walked(g, before, (what, kw, "rows"))
    same_rows(res, want[0], want[1], (what, kw))
    if keep is None:
        before = ctr(g)
        st, cnt, ck = g.query_batch_stats(ranges, impg_amd.make_params(**kw))
        walked(g, before, (what, kw, "stats"))
        g.set_option("walk_kernel", 0)
        before = ctr(g)
        st0, cnt0, ck0 = g.query_batch_stats(ranges, impg_amd.make_params(**kw))
        declined(g, before, (what, kw, "walk_kernel 0"))
        g.set_option("walk_kernel", 1)
        assert (cnt.tolist(), ck.tolist(), st.projected) == (cnt0.tolist(), ck0.tolist(), st0.projected), (what, kw)
        assert st.projected == want[1], (what, kw)
    return want


def ranges_of(g, queries):
    return [(g.seq_id(t), s, e) for t, s, e in queries]


# ---- 1. the fixtures ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, c in dg.CASES.items() if c.multi])
def test_dfs_gen_multi_fixtures(tmp_path, name):
    """This test fails without the arm: walk_launches does not move for a MultiImpg call."""
    case = dg.CASES[name]
    g, c = both(tmp_path, case.texts)
    ranges = ranges_of(g, case.queries)
    for kw in case.kws:
        for dfs in ENDS:
            by_the_walk(g, c, ranges, dict(kw, dfs=dfs), what=name)


@pytest.mark.parametrize("name", list(mg.FIXTURES))
def test_fixture(tmp_path, name):
    fx = mg.FIXTURES[name]
    g, c = both(tmp_path, fx.texts)
    ranges = ranges_of(g, fx.queries)
    keep = keep_of(c, fx.keep)
    for kw in fx.kws:
        for dfs in ENDS:
            p = dict(kw, dfs=dfs)
            by_the_walk(g, c, ranges, p, keep, what=name)
            for r in ranges:  # ... and one range a call, the trait's shape
                by_the_walk(g, c, [r], p, keep, what=(name, r))


# ---- 2. more queries than workgroups to start with ------------------------------------------------------------------------------------
def test_ladder_batch(tmp_path):
    case = dg.CASES["ladder-300"]
    g, c = both(tmp_path, case.texts)
    ranges = ranges_of(g, case.queries)
    for depth in (2, 0):
        for dfs in ENDS:
            want = by_the_walk(g, c, ranges, mg.P(depth, dfs=dfs), what="ladder-300")
            if depth == 0:
                assert len({len(w) for w in want[0]}) > 100  # the queries die after different numbers of pops


# ---- 3. a random index ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_index(tmp_path_factory):
    return both(tmp_path_factory.mktemp("random"), mg.random_texts(), bidirectional=True)


@pytest.mark.parametrize("k", range(len(mg.RANDOM_KWS)))
def test_random_index(random_index, k):
    g, c = random_index
    kw, filtered = mg.RANDOM_KWS[k]
    keep = keep_of(c, mg.RANDOM_KEEP) if filtered else None
    ranges = ranges_of(g, mg.random_queries())
    for dfs in ENDS:
        p = dict(kw, dfs=dfs)
        want = by_the_walk(g, c, ranges, p, keep, what=("random", k))
        g.set_option("walk_kernel", 1)
        for i, r in enumerate(ranges):  # one range a call: rows only (the reference is computed once, above)
            before = ctr(g)
            res = g.query_batch([r], impg_amd.make_params(**p), subset_keep=keep)
            walked(g, before, ("random", k, dfs, i))
            assert res[0].tolist() == want[0][i].tolist(), ("random", k, dfs, i)


# ---- 4. the fallback answers ----------------------------------------------------------------------------------------------------------
def next_multi_query(g, c, dfs):
    r = (g.seq_id(wg.SIDE_RANGE[0]),) + wg.SIDE_RANGE[1:]
    kw = mg.P(3, min_transitive_len=10, dfs=dfs)
    want = by_the_walk(g, c, [r], kw, what="next query")
    assert len(want[0][0]) > 3


@pytest.mark.parametrize("text,n,bit,kw,ends", [(wg.pile, mg.PAIRS_STAYS, 0, mg.PAIRS_KW, ENDS), (wg.pile, mg.PAIRS_FALLS, wg.PAIRS, mg.PAIRS_KW, ENDS),
                                               (wg.spread, mg.STACK_STAYS, 0, mg.STACK_KW, (True,)), (wg.spread, mg.STACK_FALLS, wg.STACK, mg.STACK_KW, (True,))])
def test_slab_limits(tmp_path, text, n, bit, kw, ends):
    g, c = both(tmp_path, [text(n)])
    g.set_option("walk_kernel", 1)
    r = (g.seq_id("T"),) + wg.PILE_RANGE[1:]
    for dfs in ends:
        p = dict(kw, dfs=dfs)
        want, proj = oracle_rows(c, [r], p)
        if not bit:
            by_the_walk(g, c, [r], p, what=(text.__name__, n), want=(want, proj))
            continue
        before = ctr(g)
        res = g.query_batch([r], impg_amd.make_params(**p))
        fell(g, before, bit, (text.__name__, n, dfs))
        same_rows(res, want, proj, (text.__name__, n, dfs))
        next_multi_query(g, c, dfs)


# ---- 5. what is still declined ------------------------------------------------------------------------------------------------------------
def test_declined(tmp_path):
    fx = mg.FIXTURES["ties"]
    g, c = both(tmp_path, fx.texts)
    g.set_option("walk_kernel", 1)
    ranges = ranges_of(g, fx.queries)
    for dfs in ENDS:
        kw = dict(fx.kws[0], dfs=dfs)
        before = ctr(g)
        res = g.query_batch(ranges, impg_amd.make_params(store_cigar=True, **kw))
        declined(g, before, "store_cigar")
        for i, (t, s, e) in enumerate(ranges):
            want, wcg = c.query_cigar(t, s, e, **kw)
            assert res[i].tolist() == want.tolist() and [x.tolist() for x in res.cigars(i)] == [x.tolist() for x in wcg], ("store_cigar", i)
        mask = {q: (c.seq_len(q), [(5020, 5040)] if c.seq_name(q) == "Q" else []) for q in range(c.num_seqs())}
        before = ctr(g)
        res = g.query_batch(ranges, impg_amd.make_params(**kw), masked_regions=mask)
        declined(g, before, "mask")
        want, proj = oracle_rows(c, ranges, kw, mask=mask)
        same_rows(res, want, proj, "mask")
        assert want[0][0].tolist() != oracle_rows(c, ranges[:1], kw)[0][0].tolist()  # (the mask shows in the rows)


def test_declined_sharded(tmp_path):
    fx = mg.FIXTURES["ties"]
    g, c = both(tmp_path, fx.texts, devices=[0, 0, 0], lanes=2)
    g.set_option("walk_kernel", 1)
    ranges = ranges_of(g, fx.queries)
    for dfs in ENDS:
        kw = dict(fx.kws[0], dfs=dfs)
        before = ctr(g)
        res = g.query_batch(ranges, impg_amd.make_params(**kw))
        declined(g, before, "sharded")
        want, proj = oracle_rows(c, ranges, kw)
        same_rows(res, want, proj, "sharded")
