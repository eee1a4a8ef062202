"""tests/multi_walk_gen.py checked without a GPU: every fixture reaches the edge it was built for, by the oracle's own answers, so
tests/test_gpu_walk_multi.py cannot silently stop sitting on one; the constants the helper mirrors are the source's; and the
inputs of the GPU test's counter conditions (no fallback on the random index; which side of a slab limit a pile lands on under
MultiImpg semantics) are ones the walk's slab can meet.  The discriminating answers are written out as literals."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as o
from tests import multi_walk_gen as mg
from tests import walk_gen as wg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "impg_amd", "csrc")
ENDS = (True, False)  # dfs: popped at the back, at the front


def src(name):
    return open(os.path.join(CSRC, name)).read()


def index(texts, tmp_path, bidirectional=False):
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ("f%d.paf" % i)))
        with open(paths[-1], "w") as f:
            f.write(t)
    return o.OracleIndex(paf_paths=paths, bidirectional=bidirectional, preparse=True)


def keep_of(c, names):
    return None if names is None else np.array([c.seq_name(i) in names for i in range(c.num_seqs())], dtype=np.uint8)


def ask(c, q, kw, dfs, keep=None):
    rows = c.query(c.seq_id(q[0]), q[1], q[2], subset_keep=keep, **dict(kw, dfs=dfs))
    return [(c.seq_name(r[0]), r[1], r[2], c.seq_name(r[3]), r[4], r[5]) for r in rows.tolist()]


def on(rows, name):
    """the rows' query-side intervals on one sequence, ascending"""
    return sorted((min(a, b), max(a, b)) for n, a, b, _, _, _ in rows if n == name)


def test_constants_are_the_sources():
    k = src("walk_device.inc")
    assert re.findall(r"constexpr uint32_t WALK_POP_BUDGET = 1u << (\d+);", k) == ["20"] and mg.POP_BUDGET == 1 << 20
    assert mg.POP_BUDGET >= 1000 * 834  # three orders above the headline probe's explored pops
    assert k.count("if (MULTI && ++pops > WALK_POP_BUDGET) { failed = true; if (tid == 0) S.flag |= 256u; break; }") == 1
    e = src("engine.cpp")
    assert e.count("if (p.multi_impg) return !masked;") == 1
    assert "256 pop budget" in e


@pytest.mark.parametrize("name", list(mg.FIXTURES))
def test_every_fixture_is_answered(tmp_path, name):
    """the worklist of either end terminates on every fixture and parameter set, with the query's own row first and more behind it"""
    fx = mg.FIXTURES[name]
    c = index(fx.texts, tmp_path)
    for kw in fx.kws:
        for dfs in ENDS:
            for q in fx.queries:
                rows = ask(c, q, kw, dfs, keep_of(c, fx.keep))
                assert rows[0] == (q[0], q[1], q[2], q[0], q[1], q[2]) and len(rows) > 1, (name, kw, dfs, q)


def test_proximity(tmp_path):
    fx = mg.FIXTURES["proximity"]
    c = index(fx.texts, tmp_path)
    assert [c.seq_name(i) for i in range(4)] == mg.PROX_ORDER
    for dfs in ENDS:
        rows = ask(c, fx.queries[0], fx.kws[0], dfs)
        assert on(rows, "X") == [(890, 990), (891, 991), (1000, 1100), (1109, 1209), (1110, 1210)]  # all five reported
        assert [r[1] > r[2] for r in rows if r[0] == "X" and r[3] == "Y"] == [True] * 4              # the four on the reverse strand
        assert on(rows, "W") == [(5890, 5990), (6000, 6100), (6110, 6210)]                          # 10 away: expanded; 9 away: not
        free = ask(c, fx.queries[0], dict(fx.kws[0], min_distance_between_ranges=9), dfs)
        assert on(free, "W") != on(rows, "W")  # (at 9 every hit is inserted: the fixture sits on the comparison)


def test_piece_lengths(tmp_path):
    fx = mg.FIXTURES["piece-lengths"]
    c = index(fx.texts, tmp_path)
    for dfs in ENDS:
        rows = ask(c, fx.queries[0], fx.kws[0], dfs)
        assert on(rows, "X") == [(0, 100)] and on(rows, "Z") == [(0, 101)] and on(rows, "W") == [(1000, 1101)]
        rows = ask(c, fx.queries[0], fx.kws[1], dfs)
        assert on(rows, "W") == [(0, 100), (1000, 1101)]  # min_transitive_len 100: the piece of 100 is pushed too


def test_self_hit_tells_the_arms_apart(tmp_path):
    fx = mg.FIXTURES["self-hit"]
    c = index(fx.texts, tmp_path)
    for kw in fx.kws:
        for dfs in ENDS:
            rows = ask(c, fx.queries[0], kw, dfs)
            assert on(rows, "S") == [(0, 100)] and on(rows, "V") == [] and on(rows, "U") == [(0, 100)], (kw, dfs)
        plain = ask(c, fx.queries[0], dict(kw, multi_impg=False), True)
        assert on(plain, "S") == [(0, 100), (500, 600)] and on(plain, "V") == []   # Impg reports the hit (and expands nothing)
        assert sorted(plain) != sorted(ask(c, fx.queries[0], kw, True))


def test_indels_cut_ops(tmp_path):
    fx = mg.FIXTURES["indels"]
    cuts = mg.op_cuts(mg.INDEL_T, 100)
    assert mg.INDEL_QUERY[1] not in cuts and mg.INDEL_QUERY[2] not in cuts and mg.spans(mg.INDEL_T)[0] == 100
    c = index(fx.texts, tmp_path)
    xcuts = mg.op_cuts(mg.INDEL_X, 1000)
    for dfs in ENDS:
        rows = ask(c, mg.INDEL_QUERY, fx.kws[0], dfs)
        x = on(rows, "X")
        assert len(x) == 2 and len(on(rows, "W")) >= 1 and len(on(rows, "V")) >= 1
        fwd = [iv for iv in x if iv[1] <= 1094]
        assert fwd and all(a not in xcuts and b not in xcuts for a, b in fwd)  # the piece on X cuts ops of X -> W at both ends
        assert {c_ for _, c_ in mg.spans(mg.INDEL_T)[2]} >= set("=XID") and {c_ for _, c_ in mg.spans(mg.INDEL_X)[2]} >= set("=XID")


TOUCH_A, TOUCH_B = [], []  # what the oracle makes of the two touching entries: found by the closed test, no projection, no row


def test_touching_entries(tmp_path):
    fx = mg.FIXTURES["touching"]
    c = index(fx.texts, tmp_path)
    Y = c.seq_id("Y")
    lines = [line.split("\t") for t in fx.texts for line in t.splitlines()]
    on_y = sorted((int(f[7]), int(f[8])) for f in lines if f[5] == "Y" and int(f[7]) < mg.FAR)
    assert on_y == [(50, 100), (120, 170), (200, 250)]  # one ends at the range's start, one starts at its end
    for dfs in ENDS:
        rows = ask(c, ("Y", 100, 200), fx.kws[0], dfs)
        proj = c.last_projection_count()
        step = c.query(Y, 100, 200, multi_impg=True)
        # what the oracle makes of the two: the closed test finds them, the projection of [100, 200) on them is its to decide
        assert (on(rows, "A"), on(rows, "B"), on(rows, "C")) == (TOUCH_A, TOUCH_B, [(0, 50)]), (on(rows, "A"), on(rows, "B"), proj)
        assert len(step) == 1 + len(TOUCH_A) + len(TOUCH_B) + 1 and proj == 1


def test_ties(tmp_path):
    fx = mg.FIXTURES["ties"]
    c = index(fx.texts, tmp_path)
    assert len(fx.texts) == 3 and all("\tY\t" in t for t in fx.texts)
    for dfs in ENDS:
        rows = ask(c, ("T", 0, 1000), fx.kws[0], dfs)
        q = [r[1:3] + r[4:6] for r in rows if r[0] == "Q" and r[3] == "Y"]
        assert q == [(5000, 5100, 100, 200), (5000, 5100, 100, 210), (5000, 5100, 300, 400), (5000, 5150, 100, 250), (7000, 7100, 600, 700)]
        assert any(r[0] == "R" for r in rows)  # the pop of Y is a transitive one (depth 1), and its hits are replayed
    # the files' own order is another one: file by file the hits come as written
    written = [(int(f[2]), int(f[3]), int(f[7]), int(f[8])) for t in fx.texts for f in (line.split("\t") for line in t.splitlines()) if f[5] == "Y" and f[0] == "Q"]
    assert written != sorted(written) and sorted(written) == q


def test_front_cursor(tmp_path):
    fx = mg.FIXTURES["front-cursor"]
    c = index(fx.texts, tmp_path)
    names = [c.seq_name(i) for i in range(c.num_seqs())]
    assert names == mg.FRONT_ORDER and names.index("Z") - names.index("M") > 64 and names.index("Z") - names.index("D1") > 64
    rows = ask(c, fx.queries[0], fx.kws[0], False)
    assert on(rows, "X") == [(0, 100), (200, 300), (400, 500)] and on(rows, "W") == [(200, 300)]  # only the middle record is explored
    assert on(rows, "D1") == [(0, 100), (500, 600)] and on(rows, "D2") == [(0, 100)] and on(rows, "ZZ") == [(0, 100), (1000, 1100)]
    # the order of the rows is the order of the pops: T, E, X:[200, 300), M, Z
    assert [r[3] for r in rows[1:]] == ["T"] * 4 + ["E"] * 4 + ["X"] + ["M"] * 2 + ["Z"]
    deeper = ask(c, fx.queries[0], fx.kws[1], False)
    assert on(deeper, "W") == [(0, 100), (200, 300), (400, 500)]  # max_depth 3: nothing is too deep to explore on X


def test_subset(tmp_path):
    fx = mg.FIXTURES["subset"]
    c = index(fx.texts, tmp_path)
    keep = keep_of(c, fx.keep)
    assert keep[c.seq_id("T")] == 0 and keep[c.seq_id("A")] == 0
    for dfs in ENDS:
        rows = ask(c, fx.queries[0], fx.kws[0], dfs, keep)
        assert on(rows, "A") == [] and on(rows, "G") == [] and on(rows, "C") == [(0, 100)]
        assert on(rows, "T") == [(0, 100), (5000, 5100)] and on(rows, "B") == [(0, 100)]  # the hit on the original target passes, and leads on
        unfiltered = ask(c, fx.queries[0], fx.kws[0], dfs)
        assert on(unfiltered, "A") == [(0, 100)] and on(unfiltered, "G") == [(0, 100)]


def test_output_length_and_identity(tmp_path):
    fx = mg.FIXTURES["output-length"]
    sub = tmp_path / "a"
    sub.mkdir()
    c = index(fx.texts, sub)
    for dfs in ENDS:
        rows = ask(c, fx.queries[0], fx.kws[0], dfs)
        assert on(rows, "X") == [] and on(rows, "Z") == [(0, 150)] and on(rows, "W") == [(0, 150)]  # X: no row, but expanded
        assert on(ask(c, fx.queries[0], fx.kws[1], dfs), "X") == [(0, 50)]
    fx = mg.FIXTURES["identity"]
    sub = tmp_path / "b"
    sub.mkdir()
    c = index(fx.texts, sub)
    for dfs in ENDS:
        rows = ask(c, fx.queries[0], fx.kws[0], dfs)
        assert on(rows, "X") == [(0, 100)] and on(rows, "W") == [(0, 100)] and on(rows, "Z") == [] and on(rows, "V") == []
        rows = ask(c, fx.queries[0], fx.kws[1], dfs)
        assert on(rows, "Z") == [(0, 100)] and on(rows, "V") == [(0, 100)]


def test_random_index_stays_inside_the_slab(tmp_path):
    """The GPU test asserts walk_fallbacks == 0 on the random index.  Bounds that hold for every pop of every run, from the oracle's
    counts.  h = the projections of a query, an upper bound of its hits.  Every insert adds at most one range to a visited list and
    the pieces it cuts are at most the ranges it merges plus one: at most 2 h pieces a query.  Pieces are cut from what the query
    has not visited and are visited from then on, so the kept ones, min_transitive_len bases or more each, are disjoint: no more
    than the index's bases / min_transitive_len of them.
      pairs of one pop   <= the entries of the fullest target sequence                              against hcap
      stack pool         a list moves to 2 (len + k) records when len + k outgrows its place, and only pushes shorten the way to
                         the next move (a pop at the front takes its record's place with it): more pushes than the list was
                         long lie between two moves, at most 4 records a pushed piece in all, and 8 for every sequence's
                         first place                                                                 against scap
      visited pool       the same rule, a hit for a piece                                            against vcap
      piece scratch      len + 2 n of a pop's groups: the visited ranges and twice the pop's hits    against gcap"""
    texts = mg.random_texts()
    n_records = sum(t.count("\n") for t in texts)
    assert 540 <= n_records <= 600 and len(texts) == 3
    c = index(texts, tmp_path, bidirectional=True)
    n = c.num_seqs()
    assert n == mg.RANDOM_SEQS and all(c.seq_len(i) == mg.RANDOM_LEN for i in range(n))
    queries = mg.random_queries()
    lens = [e - s for _, s, e in queries]
    assert len(queries) == 128 and min(lens) >= 1 and max(lens) <= 5000 and min(lens) < 100 and max(lens) > 4000
    fullest = max(len(c.target_entries(t)) for t in range(n))
    assert fullest <= wg.WAVE["hcap"] and fullest < (1 << wg.SLOT_BITS)
    deepest = 0
    for kw, filtered in mg.RANDOM_KWS:
        keep = keep_of(c, mg.RANDOM_KEEP) if filtered else None
        worst = 0
        for dfs in ENDS:
            for q in queries:
                rows = c.query(c.seq_id(q[0]), q[1], q[2], subset_keep=keep, **dict(kw, dfs=dfs))
                worst = max(worst, c.last_projection_count())
                assert len(rows) < wg.ROW_REGION
        pieces = min(2 * worst, n * mg.RANDOM_LEN // kw["min_transitive_len"])
        assert 8 * n + 4 * pieces <= wg.WAVE["scap"] and 8 * n + 4 * worst <= wg.WAVE["vcap"], (kw, worst, pieces)
        assert worst + 2 * fullest <= wg.WAVE["gcap"] and pieces <= mg.POP_BUDGET and min(pieces, 2 * fullest) <= wg.WAVE["wcap"], (kw, worst)
        deepest = max(deepest, worst)
    assert deepest > 1000  # (the walks are no single steps)


@pytest.mark.parametrize("n", [mg.PAIRS_STAYS, mg.PAIRS_FALLS])
def test_pairs_limit_under_multi_semantics(n):
    o.set_sorted_visits(False)
    c = o.OracleIndex(paf_text=wg.pile(n), bidirectional=False, preparse=True)
    T = c.seq_id("T")
    for dfs in ENDS:
        rows = c.query(T, *wg.PILE_RANGE[1:], **dict(mg.PAIRS_KW, dfs=dfs))
        assert c.last_projection_count() == n and len(rows) == n + 1  # the closed test finds no more, the self-skip drops none
    assert (n > wg.WAVE["hcap"]) == (n == mg.PAIRS_FALLS)
    side = c.query(c.seq_id(wg.SIDE_RANGE[0]), *wg.SIDE_RANGE[1:], **mg.P(3, min_transitive_len=10))
    assert len(side) > 3  # the "next ordinary query"


@pytest.mark.parametrize("n", [mg.STACK_STAYS, mg.STACK_FALLS])
def test_stack_limit_under_multi_semantics(n):
    c = o.OracleIndex(paf_text=wg.spread(n), bidirectional=False, preparse=True)
    rows = c.query(c.seq_id("T"), *wg.PILE_RANGE[1:], **dict(mg.STACK_KW, dfs=True))
    assert c.last_projection_count() == 2 * n and len(rows) == 1 + 2 * n and len(set(rows["query_id"].tolist())) == 1 + 2 * n
    assert (mg.stack_use(n) > wg.WAVE["scap"]) == (n == mg.STACK_FALLS) and c.num_seqs() <= 65536
    assert mg.stack_use(mg.STACK_STAYS) == 65528 and mg.stack_use(mg.STACK_FALLS) == 65544
