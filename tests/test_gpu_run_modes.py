"""A run that is abandoned or a call that is stopped leaves nothing on its engine that the next call inherits.

The modes of a run (kept levels in any order, ordered rows placed by slot, rows left with the owning ranks) and the row
stream's kernels-done hook travel with the run's request; the engine holds a copy only while Engine::run lasts.  Every
case here ends a run early -- Engine::run left by its SplitBatch exit, a consumer's stop; never a fault -- and then asks
the same handle (one GPU, so the last-in-first-out engine pool hands the same engine back) for answers the oracle knows.

(IMPG_E_UNSUPPORTED "a single range exceeds the pair budget" cannot be provoked: Engine::run throws SplitBatch only for a
chunk of several ranges -- split_ok = n > 1 -- and a range alone runs whatever it needs.  What a pile range over the
budget does provoke is the exit that refusal would have taken: its chunk's run is abandoned mid-level, in the layout's
mode, and retried in halves down to the range alone.  The cases assert that, and the answers.)

The index: 300 random records on 6 sequences of 20 000 bp, plus a pile of 1 500 records on s0 starting in [8000, 8400)
whose query sides lie in [15000, 20000) of s3..s5.  One range over the pile makes 1 500 level-0 pairs, more than
pair_budget = 1024 (the option's minimum); the ordinary ranges are short, away from both ends of the pile, and stay below
it at both levels of a depth-2 walk (checked on the CPU in the fixture, from the PAF text and the oracle's rows)."""
import numpy as np
import pytest

import impg_amd
from impg_amd import _lib
from tests.paf_gen import random_cigar, random_paf, random_ranges, spans
from tests.proj_worker import build_index, check_forms

pytestmark = pytest.mark.gpu

L = 20000
N_PILE, PILE_LO, PILE_HI = 1500, 8000, 8400
PILE_SPAN = (7900, 10500)
BUDGET_MIN, BUDGET_DEFAULT = 1024, 1 << 28
PLAIN = dict()
BFS2 = dict(transitive=True, max_depth=2, min_transitive_len=20, min_distance_between_ranges=0)
LAYOUTS = [_lib.ROWS_ATTRIBUTED, _lib.ROWS_ORDERED, _lib.ROWS_ORDERED_SLOTS]


def pile_lines(rng):
    """N_PILE records on s0 starting in [PILE_LO, PILE_HI), both strands, 20..60 ops, query sides at the far end of s3..s5
    (the shape of pile() in test_gpu_projection_paths.py, on sequences of 20 000 bp)."""
    lines = []
    for k in range(N_PILE):
        ops = random_cigar(rng, int(rng.integers(20, 61)))
        td, qd = spans(ops)
        ts, qs = int(rng.integers(PILE_LO, PILE_HI)), int(rng.integers(15000, L - qd))
        cg = "".join("%d%s" % (ln, c) for ln, c in ops)
        lines.append("s%d\t%d\t%d\t%d\t%s\ts0\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%s" %
                     (3 + k % 3, L, qs, qs + qd, "+-"[k % 2], L, ts, ts + td, td, td + qd, cg))
    return lines


def entries_of(text, sid):
    """{sequence id: int64[n, 2]} -- the (start, end) of every index entry on it: a record's target side, and (the index is
    bidirectional) its query side."""
    ent = {i: [] for i in sid.values()}
    for ln in text.splitlines():
        f = ln.split("\t")
        ent[sid[f[5]]].append((int(f[7]), int(f[8])))
        ent[sid[f[0]]].append((int(f[2]), int(f[3])))
    return {i: np.array(v, dtype=np.int64).reshape(-1, 2) for i, v in ent.items()}


def pairs(ent, t, s, e):
    a = ent[t]
    return int(((a[:, 0] < e) & (a[:, 1] > s)).sum())


def choose_ranges(c, text, sid):
    """The pile range and 40 ordinary ranges: short, off the pile (s0 around [8000, 10000)) and off its query sides (s3..s5
    from 14500 on), each under a quarter of the smallest budget at level 0 and at the level its hits open (at most the entries
    under every hit's query side: the frontier before merging and pruning) -- a chunk of four never outgrows the budget.
    The pile range alone is over it."""
    ent = entries_of(text, sid)
    pile_range = (sid["s0"],) + PILE_SPAN
    assert pairs(ent, *pile_range) > BUDGET_MIN and len(c.query(*pile_range)) - 1 > BUDGET_MIN
    far = [sid["s3"], sid["s4"], sid["s5"]]

    def fits(r):
        t, s, e = r
        if (t == sid["s0"] and e > 7000 and s < 11000) or (t in far and e > 14500) or pairs(ent, *r) >= BUDGET_MIN // 4:
            return False
        lo_hi = [(int(h["query_id"]), min(int(h["q_first"]), int(h["q_last"])), max(int(h["q_first"]), int(h["q_last"]))) for h in c.query(*r)[1:]]
        return sum(pairs(ent, *x) for x in lo_hi) < BUDGET_MIN // 4

    ordinary = [r for r in random_ranges(33, 400, 6, L, max_len=400, min_len=60) if fits(r)][:40]
    assert len(ordinary) == 40
    return pile_range, ordinary


def options(g):
    g.set_option("locality_min", 1)
    g.set_option("fuse_final_level", 1)
    g.set_option("walk_kernel", 0)  # (small transitive batches stay on the batch engine, whose modes are the subject)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    text, names = random_paf(31, 300, n_seq=6, seq_len=L)
    text += "\n".join(pile_lines(np.random.default_rng(32))) + "\n"
    d = str(tmp_path_factory.mktemp("modes"))
    g, c = build_index(d, text)
    fresh, _ = build_index(d, text)  # never sees an abandoned run or a stopped call
    sid = {n: g.seq_id(n) for n in names}
    pile_range, ordinary = choose_ranges(c, text, sid)
    # the follow-up batches.  Plain: 100 ranges that each cover the whole pile -- 150 000 pairs on 3 600 entries, a dense
    # level (>= 32 pairs per entry) if it is fused and a sparse one (< 128) if it is listed, so a kept final level that
    # inherited keep_any_order runs on another projection kernel -- and the ordinary ranges behind them.
    rng = np.random.default_rng(34)
    cover = [(sid["s0"], int(rng.integers(7000, 7950)), int(rng.integers(10400, 12000))) for _ in range(100)]
    batches = {"plain": (cover + ordinary, PLAIN), "bfs": (ordinary + [pile_range], BFS2)}
    for h in (g, fresh):
        options(h)
    cache = {}
    fresh_arms = {k: check_forms(fresh, c, rl, kw, cache=cache, tag="fresh") for k, (rl, kw) in batches.items()}
    assert fresh_arms["plain"]["batch"] != fresh_arms["plain"]["attributed"]  # (the kept final level: listed / fused)
    return dict(g=g, c=c, ordinary=ordinary, pile_range=pile_range, batches=batches, cache=cache, fresh_arms=fresh_arms)


def follow_up(w, what):
    """The same handle after the interrupted call: every result form of both batches against the oracle -- query_batch's
    rows, query_batch_stats' counts and checksums, the attributed rows and their check(), both ordered layouts (check()
    reads the attributed layout only: the ordered rows are compared with the oracle's, row by row) -- each on the
    projection kernels the fresh handle ran it on."""
    for key, (rl, kw) in w["batches"].items():
        arms = check_forms(w["g"], w["c"], rl, kw, cache=w["cache"], tag=what)
        assert arms == w["fresh_arms"][key], (what, key, arms, w["fresh_arms"][key])


@pytest.mark.parametrize("mode", ["plain", "bfs"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_abandoned_runs_leave_no_mode_behind(world, layout, mode):
    """query_batch_device under the smallest pair budget, the pile range in the third chunk of four ranges: the two chunks
    ahead run in the layout's mode, the pile's chunk is abandoned (SplitBatch) and halved twice, until the pile range is a
    chunk of its own.  The call's rows and the calls that follow on the same engine answer as the oracle does, the latter
    on the projection kernels a fresh handle uses.  N_PILE = 1 500 gives the pile range 1 537 level-0 pairs (> 1 024)."""
    g, c, kw = world["g"], world["c"], PLAIN if mode == "plain" else BFS2
    ordinary, form = world["ordinary"], {_lib.ROWS_ATTRIBUTED: "attributed", _lib.ROWS_ORDERED: "ordered", _lib.ROWS_ORDERED_SLOTS: "slots"}[layout]
    mixed = ordinary[:9] + [world["pile_range"]] + ordinary[9:12]
    g.set_option("pair_budget", BUDGET_MIN)
    g.set_option("chunk_ranges", 4)
    try:
        dr = g.query_batch_device(mixed, impg_amd.make_params(**kw), layout=layout)
        chunks = sorted({(int(d.first_range), int(d.n_ranges)) for d in dr.parts()})
        dr.free()
        # (thirteen ranges: 8..11 halved twice, and the chunk size stays at one for the range behind them)
        assert chunks == [(0, 4), (4, 4), (8, 1), (9, 1), (10, 1), (11, 1), (12, 1)], chunks
        check_forms(g, c, mixed, kw, forms=(form,), cache=world["cache"], tag=("split", layout, mode))
    finally:
        g.set_option("pair_budget", BUDGET_DEFAULT)
        g.set_option("chunk_ranges", 0)
    follow_up(world, (layout, mode))


@pytest.mark.parametrize("mode", ["plain", "bfs"])
def test_stopped_stream_leaves_no_hook_behind(world, mode):
    """A row stream whose consumer stops it on the second of five chunks returns without raising; the next stream on the
    handle runs to its end and delivers, in range order, the rows query_batch and the oracle give."""
    g, c, ranges = world["g"], world["c"], world["ordinary"]
    kw = PLAIN if mode == "plain" else BFS2
    p = impg_amd.make_params(**kw)
    calls = []

    def stop_at_second(first, q):
        calls.append(first)
        return len(calls) == 2

    g.query_batch_stream(ranges, stop_at_second, p, chunk_ranges=8)
    assert calls == [0, 8]
    got = {}

    def collect(first, q):
        for i in range(len(q)):
            got[first + i] = np.array(q[i]).tolist()

    g.query_batch_stream(ranges, collect, p, chunk_ranges=8)
    res = g.query_batch(ranges, p)
    assert sorted(got) == list(range(len(ranges)))
    for i, (t, s, e) in enumerate(ranges):
        assert got[i] == res[i].tolist() == c.query(t, s, e, **kw).tolist(), (mode, i)
    follow_up(world, ("stream", mode))
