"""The per-query walk (walk_device.inc, Engine::run_walk, walk_two_pass) on both sides of every limit of its slab, and its
fallback proved to answer.

tests/walk_gen.py builds one small index per case and says, from the slab's capacities alone, which side of which limit the
case's query lands on; tests/test_walk_gen_cpu.py holds those capacities to the source and the fixtures to the oracle.  Here:

  stays   walk_launches rose, walk_fallbacks did not, walk_overflow == 0; rows equal the oracle's, in order.
  falls   walk_fallbacks rose and walk_launches did not, on that call; walk_overflow has the case's bit and none of 1, 64,
          128; rows equal the oracle's, in order; counts, checksums and `projected` of query_batch_stats equal the same call
          under walk_kernel 0; and the next ordinary query on the same handle is answered by the walk, with the oracle's rows
          -- a fallback must not leave the slabs or the counters poisoned.

Every falling case goes through query_batch_stats, query_batch and the single-range query_transitive_{bfs,dfs}; A also as a
DFS batch of 100 ranges (regions of no rows: counted first) of which one sits on the pile; E also by the route `partition`
takes (PartitionSession.window -> query_rows_device), on both sides.  query_batch_stats takes no mask: the H cases leave it out.
Where a falling case shows more bits than its own they are recorded in the assertion's message, the case's bit is asserted.

One-character mutations of the kernel and the cases that catch them.  The first and the third were run together on an
MI355X (both only make the walk give up earlier: nothing is written that was not before) and failed exactly A-stays and
B-stays (overflow 2), and C-stays (overflow 16); the others are judged from the code and the fixtures' arithmetic -- they
let a query write past a slab, or never end, which is not for a shared machine:
  `P > A.hcap` -> `P >= A.hcap` (the step check)          A-stays, B-stays fall (P == hcap)                           run
  `P > A.hcap` -> hcap one larger                         A-falls, B-falls stay: 4 097 pairs in arrays of 4 096       reasoned
  `dst + np > A.wcap` -> `>=`                              C-stays falls (16 384 pieces == wcap)                        run
  `P + tot > A.hcap` -> `>=` (walk_final_level)            E-stays falls, and its partition route                      reasoned
  `mlen + 1u > A.wcap` -> `mlen > A.wcap`                  H-*-falls stay (wcap + 1 self pieces in wa[wcap])            reasoned
  `len + n > cap` -> `>=` (a list's move)                  V-pool's second place moves: 16 + 40 000 + 80 000 fits, V stays  reasoned
  `sub = max(1u, s_n >> 1)` -> `s_n >> 0`                  D, F never end; `>> 2` still passes: the cut may be finer    reasoned
  `run + e < row_cap` -> `<=` (rows of the last level)     F's batch of 3: the row past a region is the next range's first  reasoned
`P >= (1u << WALK_SLOT_BITS)` -> `>` is caught by nothing alone: hcap = 2^15 - 1 is the same bound (the CPU test pins both).
"""
import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import partition_ref as pr
from tests import walk_gen as wg

pytestmark = pytest.mark.gpu
ORDER = dict(sorted=impg_amd.ORDER_SORTED, coitrees=impg_amd.ORDER_COITREES)


@pytest.fixture(autouse=True)
def reference_order_afterwards():
    yield
    o.set_sorted_visits(False)


def both(tmp_path, text, order, options):
    path = str(tmp_path / "w.paf")
    with open(path, "w") as f:
        f.write(text)
    g = impg_amd.GpuImpg.from_paf(path, bidirectional=False, order=ORDER[order])
    c = o.OracleIndex(paf_paths=[path], bidirectional=False, preparse=True)
    o.set_sorted_visits(order == "sorted")
    assert [g.seq_name(i) for i in range(g.num_seqs())] == [c.seq_name(i) for i in range(c.num_seqs())]
    for k, v in options.items():
        g.set_option(k, v)
    return g, c


def ctr(g):
    return {k: g.counter(k) for k in ("walk_launches", "walk_fallbacks", "walk_overflow")}


def stayed(g, before, launches=None, what=None):
    after = ctr(g)
    assert after["walk_launches"] > before["walk_launches"] and after["walk_fallbacks"] == before["walk_fallbacks"], (what, before, after)
    assert after["walk_overflow"] == 0, (what, after)
    if launches is not None:
        assert after["walk_launches"] - before["walk_launches"] == launches, (what, before, after)


def fell(g, before, bit, what=None):
    after = ctr(g)
    ov = after["walk_overflow"]
    others = ov & ~bit
    assert after["walk_fallbacks"] > before["walk_fallbacks"] and after["walk_launches"] == before["walk_launches"], (what, before, after)
    assert ov & bit and not others & wg.NEVER, (what, "overflow 0x%x, beside the case's bit: 0x%x" % (ov, others))
    return ov


def rid(g, rng):
    return (rng[0] if isinstance(rng[0], int) else g.seq_id(rng[0]), rng[1], rng[2])


def oracle_rows(c, r, mask, **kw):
    rows = c.query(r[0], r[1], r[2], masked_regions=mask, **kw)
    return rows, c.last_projection_count()


def same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    quick = got.dtype == want.dtype and bool(np.all(got == want))  # (140 000 rows: lists only when they are needed)
    assert quick or got.tolist() == want.tolist(), what


def single(g, r, mask, kw):
    fn = g.query_transitive_dfs if kw["dfs"] else g.query_transitive_bfs
    return fn(r[0], r[1], r[2], masked_regions=mask, max_depth=kw["max_depth"], min_transitive_len=kw["min_transitive_len"],
              min_distance_between_ranges=kw["min_distance_between_ranges"])


def next_ordinary_query(g, c, case, mask=None):
    """... is answered by the walk, with the oracle's rows"""
    r = rid(g, wg.SIDE_RANGE)
    kw = dict(transitive=True, dfs=case.dfs, **wg.SIDE_KW)
    before = ctr(g)
    res = g.query_batch([r], impg_amd.make_params(**kw), masked_regions=mask)
    stayed(g, before, what=(case.name, "next query"))
    want, proj = oracle_rows(c, r, mask, **kw)
    same(res[0], want, (case.name, "next query"))
    assert res.projected == proj and len(want) > 3


def mask_of(g, case):
    """every sequence in the map (one the map does not hold has length 0 there: nothing of it could be queried), T's list long"""
    if not case.mask:
        return None
    m = {q: (wg.SEQ_LEN, []) for q in range(g.num_seqs())}
    m[g.seq_id("T")] = (wg.SEQ_LEN, wg.mask_list(case.mask))
    return m


def run_stays(g, c, case, kw):
    p = case.params(kw)
    r, mask = rid(g, case.range), mask_of(g, case)
    want, proj = oracle_rows(c, r, mask, **p)
    launches = 2 if len(want) > wg.ROW_REGION else 1  # (more rows than the region: counted, then walked again -- E'-stays, as F)
    before = ctr(g)
    res = g.query_batch([r], impg_amd.make_params(**p), masked_regions=mask)
    stayed(g, before, launches, (case.name, kw))
    same(res[0], want, (case.name, kw))
    assert res.projected == proj
    if not mask:
        before = ctr(g)
        st, cnt, ck = g.query_batch_stats([r], impg_amd.make_params(**p))
        stayed(g, before, 1, (case.name, kw, "stats"))
        assert int(cnt[0]) == len(want) - 1 and st.projected == proj  # (the range's own row is not a hit)
        g.set_option("walk_kernel", 0)
        st0, cnt0, ck0 = g.query_batch_stats([r], impg_amd.make_params(**p))
        g.set_option("walk_kernel", case.options["walk_kernel"])
        assert (cnt.tolist(), ck.tolist(), st.projected) == (cnt0.tolist(), ck0.tolist(), st0.projected), (case.name, kw)
    return want


def run_falls(g, c, case, kw, entries=("stats", "batch", "single")):
    p = case.params(kw)
    r, mask = rid(g, case.range), mask_of(g, case)
    want, proj = oracle_rows(c, r, mask, **p)
    seen = {}
    if "stats" in entries and not mask:
        before = ctr(g)
        st, cnt, ck = g.query_batch_stats([r], impg_amd.make_params(**p))
        seen["stats"] = fell(g, before, case.bit, (case.name, kw, "stats"))
        g.set_option("walk_kernel", 0)
        st0, cnt0, ck0 = g.query_batch_stats([r], impg_amd.make_params(**p))
        g.set_option("walk_kernel", case.options["walk_kernel"])
        assert (cnt.tolist(), ck.tolist(), st.projected) == (cnt0.tolist(), ck0.tolist(), st0.projected), (case.name, kw)
        assert st.projected == proj
        next_ordinary_query(g, c, case)
    if "batch" in entries:
        before = ctr(g)
        res = g.query_batch([r], impg_amd.make_params(**p), masked_regions=mask)
        seen["batch"] = fell(g, before, case.bit, (case.name, kw, "batch"))
        same(res[0], want, (case.name, kw, "batch"))
        assert res.projected == proj
        next_ordinary_query(g, c, case, mask)
    if "single" in entries:
        before = ctr(g)
        rows = single(g, r, mask, p)
        seen["single"] = fell(g, before, case.bit, (case.name, kw, "single"))
        same(rows, want, (case.name, kw, "single"))
        next_ordinary_query(g, c, case, mask)
    assert len(set(seen.values())) == 1, seen  # every entry point meets the same cause
    return want


@pytest.mark.parametrize("name", list(wg.CASES))
def test_limit(tmp_path, name):
    case = wg.CASES[name]
    g, c = both(tmp_path, case.text(), case.order, case.options)
    for kw in case.kws:
        if case.bit:
            run_falls(g, c, case, kw)
        else:
            run_stays(g, c, case, kw)
            next_ordinary_query(g, c, case, mask_of(g, case))


def test_dfs_batch_of_100_falls_as_a_whole(tmp_path):
    """A, as a batch of more than 64 ranges (regions of no rows: the walk counts first): one range sits on the pile of 4 097, the
    whole batch goes to the batch engine, all 100 answers equal the oracle's."""
    case = wg.CASES["A-falls"]
    g, c = both(tmp_path, case.text(), case.order, case.options)
    p = case.params(dict(wg.SIDE_KW, max_depth=2))
    U, V = g.seq_id("U"), g.seq_id("V")
    ranges = [((U, V)[i & 1], 37 * i, 37 * i + 400 + 11 * i) for i in range(99)]
    ranges.insert(41, (g.seq_id("T"), 1000, 1100))
    assert len(ranges) > wg.SMALL_RANGES
    before = ctr(g)
    res = g.query_batch(ranges, impg_amd.make_params(**p))
    fell(g, before, case.bit)
    total = 0
    for i, r in enumerate(ranges):
        want, proj = oracle_rows(c, r, None, **p)
        same(res[i], want, (i, r))
        total += proj
    assert res.projected == total and len(res[41]) == 4098
    before = ctr(g)
    small = g.query_batch(ranges[:41] + ranges[42:], impg_amd.make_params(**p))  # the same batch without the pile: the walk's
    stayed(g, before, 2)  # (counted, then placed)
    assert [small[i].tolist() for i in range(99)] == [res[i].tolist() for i in range(100) if i != 41]


@pytest.mark.parametrize("form", list(wg.D_FORMS))
def test_level_cut_into_sub_steps(tmp_path, form):
    """D: fan(40, 1000) -- level 2 is 40 000 pairs, more than a step holds, so it is halved (20 ranges a step); the visited
    updates between the sub-steps must be exact.  One workgroup and the grid form (2, 5 members: the leader cuts level 2, the
    last level is shared), a depth limit and none, and a proximity test under which the order of a level's hits shows in the
    pieces; in the reference's visit order."""
    g, c = both(tmp_path, wg.fan(*wg.D_FAN), "coitrees", wg.D_FORMS[form])
    r = rid(g, wg.PILE_RANGE)
    for kw in wg.D_KWS:
        p = dict(transitive=True, **kw)
        want, proj = oracle_rows(c, r, None, **p)
        before = ctr(g)
        res = g.query_batch([r], impg_amd.make_params(**p))
        stayed(g, before, 1, (form, kw))
        same(res[0], want, (form, kw))
        assert res.projected == proj
        if kw["max_depth"] >= 2:
            assert g.counter("walk_members") == wg.D_FORMS[form]["walk_members"]


@pytest.mark.parametrize("form", list(wg.F_FORMS))
def test_rows_beyond_the_region_are_walked_twice(tmp_path, form):
    """F (and E' on its staying side under 5 members): fan(140, 1000) -- 140 141 rows > 2^17, so walk_two_pass counts, then
    walks again at the exact size: two launches, no fallback, the oracle's rows.  Also as a batch of 3 ranges of which only one
    outgrows its region."""
    g, c = both(tmp_path, wg.fan(*wg.F_FAN), "coitrees", wg.F_FORMS[form])
    r = rid(g, wg.PILE_RANGE)
    for kw in wg.F_KWS:
        p = dict(transitive=True, **kw)
        want, proj = oracle_rows(c, r, None, **p)
        assert len(want) > wg.ROW_REGION
        before = ctr(g)
        res = g.query_batch([r], impg_amd.make_params(**p))
        stayed(g, before, 2, (form, kw))
        same(res[0], want, (form, kw))
        assert res.projected == proj
    batch = [rid(g, wg.SIDE_RANGE), r, (g.seq_id("V"), 900, 1600)]
    p = dict(transitive=True, **wg.F_KWS[0])
    before = ctr(g)
    res = g.query_batch(batch, impg_amd.make_params(**p))
    stayed(g, before, 2, (form, "batch of 3"))
    for i, b in enumerate(batch):
        want, _ = oracle_rows(c, b, None, **p)
        same(res[i], want, (form, "batch of 3", i))
    before = ctr(g)
    st, cnt, ck = g.query_batch_stats(batch, impg_amd.make_params(**p))
    stayed(g, before, 1)
    assert cnt.tolist() == [len(res[i]) - 1 for i in range(3)]


@pytest.mark.parametrize("name", ["E-stays", "E-falls"])
def test_partition_route(tmp_path, name):
    """query_rows_device, the route `partition` takes, through PartitionSession.window: a fresh session's first window is the
    case's range (every sequence masked by an empty list), its second the ordinary one -- against the oracle's rows put
    through the restated window algebra."""
    case = wg.CASES[name]
    g, c = both(tmp_path, case.text(), case.order, case.options)
    p = case.params(case.kws[0])
    n = c.num_seqs()
    lens = [c.seq_len(q) for q in range(n)]
    ref = pr.Ref(lens)
    s = g.partition_session(1000, 0, impg_amd.make_params(**p), min_missing_size=0, min_boundary_distance=0)
    try:
        for k, rng in enumerate((case.range, wg.SIDE_RANGE)):
            r = rid(g, rng)
            mask = {q: (lens[q], ref.masked.get(q)) for q in range(n)}
            rows, _ = oracle_rows(c, r, mask, **p)
            want = ref.apply([(int(x["query_id"]), int(x["q_first"]), int(x["q_last"])) for x in rows], 0, 0, 0)
            before, walked = ctr(g), s.counter("walk_windows")
            got = s.window(*r, cap=1 << 12)
            if k == 0 and case.bit:
                fell(g, before, case.bit, name)
                assert s.counter("walk_windows") == walked
            else:
                stayed(g, before, 1, (name, k))
                assert s.counter("walk_windows") == walked + 1
            assert got == want and len(want) > 0, (name, k)
    finally:
        s.close()
