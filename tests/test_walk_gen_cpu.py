"""tests/walk_gen.py checked without a GPU: the constants it mirrors are the source's, and the oracle agrees with every
fixture's arithmetic -- so tests/test_gpu_walk_limits.py cannot silently stop sitting on an edge.

(The oracle's DFS re-sorts its stack after every pop: quadratic in a pile's size, so DFS runs here only on piles of about
5 000 or fewer; its BFS takes a 32 768-hit window in a few hundredths of a second.)"""
import os
import re

import pytest

from oracle import oracle as o
from tests import walk_gen as wg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "impg_amd", "csrc")


def src(name):
    return open(os.path.join(CSRC, name)).read()


def test_constants_are_the_sources():
    """Engine::walk_caps, WALK_SLOT_BITS, SMALL_RANGES and both 2^17-row regions, read from the text: a changed cap fails here."""
    body = re.search(r"void Engine::walk_caps\(bool wide, WalkArgs &a\) \{(.*?)\n\}", src("engine.cpp"), re.S).group(1)
    caps = re.findall(r"a\.(\w+) = wide \? (\d+)u : (\d+)u;", body)
    assert len(caps) == 5 and len(re.findall(r"a\.\w+\s*=", body)) == 5, body
    assert {k: int(w) for k, w, _ in caps} == wg.WIDE and {k: int(v) for k, _, v in caps} == wg.WAVE
    assert re.findall(r"constexpr uint32_t WALK_SLOT_BITS = (\d+);", src("walk_device.inc")) == [str(wg.SLOT_BITS)]
    assert re.findall(r"SMALL_RANGES = (\d+),", src("engine.hpp")) == [str(wg.SMALL_RANGES)]
    capi = src("capi.cpp")
    regions = re.findall(r"1u << (\d+)", capi[capi.index("bool walk_query("):capi.index("void check_ranges(")])
    assert regions == ["17", "17"] and wg.ROW_REGION == 1 << 17  # walk_query's and query_rows_device's
    # the comparisons the cases sit on, as the kernel writes them (a mutation of one of them must fail a GPU case, see there)
    k = src("walk_device.inc")
    for text in ("if (P > A.hcap || P >= (1u << WALK_SLOT_BITS)) {", "if (P + tot > A.hcap) { fine = false; break; }",
                 "if (dst + np > A.wcap) { atomicOr(&S.flag, 16u); continue; }", "if (noff + ncap > A.vcap) { atomicOr(&S.flag, 4u); continue; }",
                 "if (po + pcap > A.gcap) { atomicOr(&S.flag, 8u); continue; }", "if (noff + ncap > A.scap) { atomicOr(&S.flag, 32u); continue; }",
                 "mlen + 1u > A.wcap", "if (n_new > A.wcap) {"):
        assert k.count(text) == 1, text


def index(text, sorted_visits=True):
    o.set_sorted_visits(sorted_visits)
    return o.OracleIndex(paf_text=text, bidirectional=False, preparse=True)


@pytest.fixture(autouse=True)
def reference_order_afterwards():
    yield
    o.set_sorted_visits(False)


def ask(c, rng, **kw):
    t, s, e = rng
    rows = c.query(c.seq_id(t), s, e, transitive=True, **kw)
    return rows, c.last_projection_count()


@pytest.mark.parametrize("n", [4096, 4097, 16384, 16385, 32767, 32768])
def test_pile(n):
    c = index(wg.pile(n))
    rows, proj = ask(c, wg.PILE_RANGE, **wg.d(1))
    assert len(rows) == n + 1 and proj == n
    Q = c.seq_id("Q")
    assert rows["query_id"][1:].tolist() == [Q] * n and rows["q_first"][1:].tolist() == [2000 * k for k in range(n)]  # input order
    rows, proj = ask(c, wg.PILE_RANGE, **wg.d(3))   # n distinct pieces, and nothing behind them
    assert len(rows) == n + 1 and proj == n
    if n <= 5000:
        rows, proj = ask(c, wg.PILE_RANGE, dfs=True, **wg.d(2))
        assert len(rows) == n + 1 and proj == n
    side, _ = ask(c, wg.SIDE_RANGE, **wg.SIDE_KW)
    assert len(side) > 3  # the "next ordinary query" has more than its own row


@pytest.mark.parametrize("places,per,depth,total", [wg.D_FAN + (3, wg.D_ROWS), wg.F_FAN + (2, wg.F_ROWS), (2, 32767, 2, 1 + 2 + 2 * 32767),
                                                    (2, 32768, 2, 1 + 2 + 2 * 32768)])
def test_fan(places, per, depth, total):
    """Level 2 holds places x per pairs, `per` per range; the row totals the GPU cases rely on."""
    c = index(wg.fan(places, per), sorted_visits=False)
    rows, proj = ask(c, wg.PILE_RANGE, **wg.d(2))
    assert proj == places + places * per and len(rows) == 1 + places + places * per
    Q, R = c.seq_id("Q"), c.seq_id("R")
    lvl2 = rows[1 + places:]
    assert set(lvl2["query_id"].tolist()) == {R} and set(lvl2["target_id"].tolist()) == {Q}
    starts, counts = zip(*sorted((int(s), int((lvl2["t_first"] == s).sum())) for s in set(lvl2["t_first"].tolist())))
    assert starts == tuple(wg.PLACE_STEP * k for k in range(places)) and set(counts) == {per}
    assert per <= wg.WIDE["hcap"] or (places, per) == (2, 32768)
    rows, proj = ask(c, wg.PILE_RANGE, **wg.d(depth))
    assert len(rows) == total
    if depth == 3:
        assert total == 40241 and proj == places + places * per + wg.R_TO_S  # R's pieces merge into one range: every R -> S alignment once
    else:
        assert total in (140141, 65537, 65539) and (total > wg.ROW_REGION) == (places == 140)


def test_fan_order_shows_in_the_pieces():
    """D's third parameter set: under a proximity test and a length cut-off the pieces depend on the order of a level's hits
    -- the two visit orders give different level-3 rows, and neither gives the plain run's."""
    text = wg.fan(*wg.D_FAN)
    plain, _ = ask(index(text, False), wg.PILE_RANGE, **wg.D_KWS[0])
    tree, _ = ask(index(text, False), wg.PILE_RANGE, **wg.D_KWS[2])
    by_start, _ = ask(index(text, True), wg.PILE_RANGE, **wg.D_KWS[2])
    assert len(plain) == wg.D_ROWS
    assert len({len(plain), len(tree), len(by_start)}) == 3, (len(plain), len(tree), len(by_start))
    unlimited, _ = ask(index(text, False), wg.PILE_RANGE, **wg.D_KWS[1])
    assert unlimited.tolist() == plain.tolist()  # (S has no way on: no depth limit, the same rows)


def test_masks():
    for m in (4095, 4096, 16383, 16384):
        ml = wg.mask_list(m)
        assert len(ml) == m and all(a < b for a, b in ml) and all(ml[i][1] < ml[i + 1][0] for i in range(m - 1))
        assert wg.MASK_RANGE[1] < ml[0][0] and ml[-1][1] < wg.MASK_RANGE[2] <= wg.SEQ_LEN
    c = index(wg.pile(50))
    T = c.seq_id("T")
    for m, dfs in ((4095, True), (16383, False)):
        rows = c.query(T, *wg.MASK_RANGE[1:], masked_regions={T: (wg.SEQ_LEN, wg.mask_list(m))}, transitive=True, dfs=dfs,
                       **wg.d(2, min_transitive_len=5))
        assert len(rows) == m + 1 + 50 and (rows["query_id"][:m + 1] == T).all()  # m + 1 self pieces, then the pile's hits


@pytest.mark.parametrize("name", list(wg.CASES))
def test_case_arithmetic(name):
    """Every case says which side it is on (Case.__init__ asserts value <= cap exactly when it stays); here the oracle
    confirms the values that are counts of hits, and the fixtures of the pool cases do what their arithmetic assumes."""
    case = wg.CASES[name]
    assert (case.bit == 0) == name.endswith("-stays")
    c = index(case.text(), case.order == "sorted")
    if case.mask:
        assert case.value == len(wg.mask_list(case.mask)) + 1
        return
    if case.fixture is wg.pile:
        rows, proj = ask(c, case.range, **wg.d(1))
        assert proj == case.value
    elif name.startswith("E"):
        rows, proj = ask(c, case.range, **wg.d(2))
        places, per = case.args
        members = case.options["walk_members"]
        share = max((places * (m + 1) // members - places * m // members) for m in range(members)) * per  # walk_final_level's r0, r1
        assert share == case.value and proj == places + places * per
    elif name == "V-pool":
        rows, proj = ask(c, case.range, **case.kws[0])
        assert proj == 3 + 60000 and len(rows) == 1 + 3 + 60000  # no piece of R is long enough: nothing reaches S
        R = c.seq_id("R")
        r = rows[rows["query_id"] == R]
        lo = [min(a, b) for a, b in zip(r["q_first"].tolist(), r["q_last"].tolist())]
        assert lo == [200 * i for i in range(60000)]  # distinct, ascending in visit order: every hit appends to R's list
    elif name == "G-scratch":
        rows, proj = ask(c, case.range, dfs=True, **case.kws[0])
        assert proj == 4 + 16000 and len(rows) == 1 + 4 + 16000
        R = c.seq_id("R")
        r = rows[rows["query_id"] == R]
        lo = [min(a, b) for a, b in zip(r["q_first"].tolist(), r["q_last"].tolist())]
        assert lo == [200 * i for i in range(16000)]  # ascending in the order the DFS replays them (Q's last place is popped first)
    elif name == "S-stack":
        rows, proj = ask(c, case.range, dfs=True, **case.kws[0])
        assert proj == 2 * 4096 and len(rows) == 1 + 2 * 4096 and len(set(rows["query_id"].tolist())) == 1 + 2 * 4096
        assert c.num_seqs() <= 65536
    else:
        raise AssertionError("a case without a check: " + name)
