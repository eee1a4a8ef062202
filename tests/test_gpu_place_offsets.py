"""A fused final level's place offsets in two levels (option place_offsets_blocks), the update's tiers launched by their
counts, and the lookup order's idx array written only for the library sort -- against the oracle and against the old path.

lookup_count_coop_kernel leaves every place's offset inside its block of 64 places (a wave's) and the blocks' sums; a scan
over the sums stands in for the scan over every range's count, and project_entries_kernel adds the two.  The engine takes that
path only for a fused level that kernel runs (a dense one) whose count pass deferred no wide window; counter
"place_offsets_block_levels" says that it did.  Every case runs with the option at 0 and at 1: equal counts, checksums and
rows, all equal to the oracle's, and the counter rises exactly where the case is built to reach the new path.

Block edges: a level's n ranges fill n / 64 waves and n / 256 blocks of the count kernel and n / 512 of the projection's.  The sizes below
are reached with the FIRST level as the final one (plain, and -x -m 1), where n is the batch's size -- read back from the
`n_frontier` of DeviceRows.parts() -- because a deeper level's size cannot be set from outside; the synthetic -x -m 3 case
covers a deeper final level at whatever size it comes to (printed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (run as the child of test_library_sort_in_a_fresh_process)
    sys.path.insert(0, ROOT)

import impg_amd  # noqa: E402
from oracle import oracle as o  # noqa: E402
from tests import update_gen as ug  # noqa: E402
from tests.proj_worker import build_index, check_forms  # noqa: E402
from tests.test_gpu_projection_paths import L, M1, covering, fused_options, pile  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = ("stats", "attributed")
BLOCK_LEVELS = "place_offsets_block_levels"
M3 = dict(transitive=True, max_depth=3)


def both_paths(g, c, ranges, kw, cache, tag, new_levels):
    """`ranges` under `kw` with place_offsets_blocks 0 and 1: every form against the oracle (check_forms), the two settings'
    per-range counts and checksums -- from query_batch_stats and from the rows in HBM -- against each other, and the new
    path's counter: no rise at 0; at 1 a rise where new_levels says so (True: some level, False: none, None: not asked)."""
    p = impg_amd.make_params(**kw)
    seen = []
    try:
        for pob in (0, 1):
            g.set_option("place_offsets_blocks", pob)
            before = g.counter(BLOCK_LEVELS)
            check_forms(g, c, ranges, kw, forms=FORMS, cache=cache, tag=(tag, pob))
            st, cnt, ck = g.query_batch_stats(ranges, p)
            dr = g.query_batch_device(ranges, p)
            dcnt, dck = dr.check()
            n_fr = [(int(d.level), int(d.n_frontier)) for d in dr.parts()]
            dr.free()
            rise = g.counter(BLOCK_LEVELS) - before
            if pob == 0:
                assert rise == 0, (tag, rise)
            elif new_levels is not None:
                assert (rise > 0) == new_levels, (tag, rise)
            assert (cnt == dcnt).all() and (ck == dck).all(), (tag, pob)
            seen.append((int(st.projected), int(st.pairs), cnt.tolist(), ck.tolist(), n_fr))
    finally:
        g.set_option("place_offsets_blocks", 1)
    assert seen[0] == seen[1], tag
    return seen[1]


# ---- old path against new path: a synthetic index, -x -m 3 -------------------------------------------------------------------
def test_synthetic_m3_old_against_new(tmp_path):
    """600 records on 6 sequences (1 200 entries), 256 ranges: the third level is the final one, some 10^5 pairs -- dense
    (32 pairs an entry is the threshold), so it is fused, runs entry by entry and takes the two-level offsets."""
    path = str(tmp_path / "s.paf")
    shape = dict(n_seq=6, seq_len=300000, target_span=10000, n_blocks=100)
    impg_amd.synth_paf_text(path, 42, 600, **shape)
    g = impg_amd.GpuImpg.from_paf(path)
    c = o.OracleIndex(paf_paths=[path], preparse=True)
    assert g.num_records() <= 2000 and g.num_seqs() <= 8
    fused_options(g)
    bed = impg_amd.synth_bed(7, 256, n_seq=6, seq_len=300000, range_len=5000)
    ranges = [(g.seq_id(impg_amd.synth_seq_name(int(r["target_id"]))), int(r["start"]), int(r["end"])) for r in bed]
    got = both_paths(g, c, ranges, M3, {}, "synthetic -x -m 3", True)
    print("synthetic -x -m 3: projected %d, pairs %d, (level, frontier) of the parts %s" % (got[0], got[1], got[4]))
    both_paths(g, c, ranges, {}, {}, "synthetic plain", None)


# ---- block edges ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pile40(tmp_path_factory):
    """40 records on T (one direction: 40 entries; Q0 .. Q7 own none), 1 025 ranges that each cover all of them."""
    rng = np.random.default_rng(7)
    text = "\n".join(pile(rng, "T", 40, 10000, 12000, ["Q%d" % i for i in range(8)])) + "\n"
    g, c = build_index(str(tmp_path_factory.mktemp("po40")), text, bidirectional=False)
    assert g.num_entries() == 40
    fused_options(g)
    return g, c, covering(g, "T", 1025, 9000, 15000, 1025), {}


SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]  # (every one of them runs: the final level is the first)


@pytest.mark.parametrize("n", SIZES)
def test_block_edges(pile40, n):
    """n ranges of 40 pairs each in the final level: the last wave of the count kernel holds n mod 64 places, its last block
    n mod 256, the projection's n mod 512 ranges, and its end is read across the border (place n is another block's first).  One range
    alone is no dense level (40 pairs on 40 entries): the sums are scanned, then the old path runs -- the fall-back by size."""
    g, c, ranges, cache = pile40
    for kw in ({}, M1):
        got = both_paths(g, c, ranges[:n], kw, cache, ("edges", n), n >= 32)
        assert kw or got[1] == 40 * n
        assert [f for _, f in got[4]] == [n], got[4]  # (one part, one level: its frontier is the batch)


def test_empty_blocks_and_empty_final_level(pile40):
    """600 ranges on Q0 and Q1, which own no entry, between the hitting ones: in the lookup order they are whole blocks of
    places without a hit (sum 0, every offset 0), and hitting ranges share blocks with them at either end.  Under
    -x -m 2 the second level is the final one and finds nothing at all: an empty fused level."""
    g, c, ranges, cache = pile40
    rng = np.random.default_rng(5)
    empty = [(g.seq_id("Q%d" % (k % 2)), int(rng.integers(0, L // 2)), int(rng.integers(L // 2, L))) for k in range(600)]
    mixed = []
    for k in range(300):
        mixed += [ranges[k], empty[2 * k], empty[2 * k + 1]]
    for kw in ({}, M1):
        got = both_paths(g, c, mixed, kw, cache, "empty blocks", True)
        assert kw or got[1] == 40 * 300
    m2 = dict(M1, max_depth=2)
    got = both_paths(g, c, mixed[:90], m2, cache, "empty final level", False)
    assert got[1] <= 40 * 30  # (the first level's pairs: the second has none)
    both_paths(g, c, empty[:300], {}, cache, "nothing hits", False)


# ---- a deferred wide window ----------------------------------------------------------------------------------------------------
def test_deferred_wide_window_takes_the_old_path(tmp_path):
    """600 narrow ranges over a 40-entry pile and one range over 100 records of another target: its window is wider than
    the hit mask, the count pass defers it (its count comes from lookup_count_wide_kernel, after the block sums), and the
    level must take the per-range scan -- the sums are short by 100.  Counter lookup_wide_windows proves the window was
    listed; the same batch without it takes the two-level offsets.  With the cooperative span and the emit buffer lowered
    as well (the lane body defers the window, the emit pass groups it) nothing changes."""
    rng = np.random.default_rng(19)
    lines = pile(rng, "T", 40, 10000, 12000, ["Q%d" % i for i in range(8)])
    lines += pile(rng, "W", 100, 10000, 10400, ["Q%d" % i for i in range(8)], min_ops=2, max_ops=8)
    g, c = build_index(str(tmp_path), "\n".join(lines) + "\n", bidirectional=False)
    assert g.num_entries() == 140
    fused_options(g, lookup_stats=1)
    narrow = covering(g, "T", 600, 9000, 15000, 600)
    wide = (g.seq_id("W"), 9000, 12000)
    ranges = narrow[:300] + [wide] + narrow[300:]
    cache = {}
    try:
        for span, cap in ((256, 4096), (16, 64)):
            g.set_option("lookup_coop_span", span)
            g.set_option("wide_emit_cap", cap)
            for kw in ({}, M1):
                before = g.counter("lookup_wide_windows")
                got = both_paths(g, c, ranges, kw, cache, ("wide", span, cap), False)
                assert kw or got[1] == 600 * 40 + 100
                assert g.counter("lookup_wide_windows") > before
                before = g.counter("lookup_wide_windows")
                both_paths(g, c, narrow, kw, cache, ("narrow", span, cap), True)
                assert g.counter("lookup_wide_windows") == before
    finally:
        g.set_option("lookup_coop_span", 256)
        g.set_option("wide_emit_cap", 4096)


# ---- the update's tiers, launched by their counts -------------------------------------------------------------------------------
TIER_KEYS = ["update_lane_groups", "update_mid_groups", "update_wave_tiny_groups", "update_wave_small_groups", "update_wave_large_groups"]
# one update (-x -m 2) of the two batches below, as the commit before this change counted them (update_stats 1)
ALL_TIERS = dict(update_lane_groups=1, update_mid_groups=1, update_wave_tiny_groups=1, update_wave_small_groups=1, update_wave_large_groups=1)
NO_LISTED_TIER = dict(update_lane_groups=1, update_mid_groups=0, update_wave_tiny_groups=0, update_wave_small_groups=0, update_wave_large_groups=0)
# (sequence, ranges it starts with, hits): cap = old + hits picks the tier (tests/update_gen.py, tier_of)
TIER_GROUPS = [("A", 0, 5), ("B", 0, 20), ("C", 0, 60), ("D", 0, 300), ("E", 900, 60)]
assert [ug.tier_of(m + h, m) for _, m, h in TIER_GROUPS] == ["lane", "mid", "tiny", "small", "large"]


def tiers_fixture(d):
    """One query range on T whose hits land on A .. E: isolated hits (update_gen.fillers), E's between the 900 ranges its
    list starts with (masked_regions).  The first 5 records are A's: a range over those alone reaches the lane tier only."""
    lines, k, gap = [], 0, 30
    lq = ug.slot(1000)[1] + 3000
    n_rec = sum(h for _, _, h in TIER_GROUPS)
    lt = 1000 + n_rec * gap + 1000
    for name, m, h in TIER_GROUPS:
        for s, e in ug.fillers(m, h):
            ts = 1000 + k * gap
            lines.append("%s\t%d\t%d\t%d\t%s\tT\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%d=" % (name, lq, s, e, "+-"[k % 2], lt, ts, ts + (e - s), e - s, e - s, e - s))
            k += 1
    g, c = build_index(d, "\n".join(lines) + "\n", bidirectional=False)
    masked = {g.seq_id("T"): (lt, [])}
    for name, m, _ in TIER_GROUPS:
        masked[g.seq_id(name)] = (lq, [ug.slot(i) for i in range(m)])
    every = [(g.seq_id("T"), 500, lt - 500)]
    lane_only = [(g.seq_id("T"), 500, 1000 + 5 * gap - 5)]
    return g, c, masked, every, lane_only


def test_tier_launches(tmp_path):
    """A batch whose groups reach the mid, tiny, small and large tiers (and the lane kernel), and one that reaches none of
    the listed ones: rows against the oracle, the groups per tier as before the tiers were launched by their counts."""
    g, c, masked, every, lane_only = tiers_fixture(str(tmp_path))
    g.set_option("walk_kernel", 0)
    g.set_option("update_stats", 1)
    kw = dict(transitive=True, min_transitive_len=ug.MTL, min_distance_between_ranges=0)
    for ranges, want in ((every, ALL_TIERS), (lane_only, NO_LISTED_TIER)):
        for depth in (2, 3):
            p = dict(kw, max_depth=depth)
            before = {k2: g.counter(k2) for k2 in TIER_KEYS}
            res = g.query_batch(ranges, impg_amd.make_params(**p), masked_regions=masked)
            rise = {k2: g.counter(k2) - before[k2] for k2 in TIER_KEYS}
            print("tiers", len(ranges), depth, rise)
            for i, (t, s, e) in enumerate(ranges):
                assert res[i].tolist() == c.query(t, s, e, masked_regions=masked, **p).tolist(), (i, depth)
            if depth == 2:  # (one update)
                assert rise == want, (rise, want)


# ---- IMPG_LIB_SORT=1: the idx array is still written there -----------------------------------------------------------------------
def lib_sort_child():
    """The child process: -x -m 2 and -m 3 over a bidirectional pile (the update writes the next level's keys beside the
    frontier; locality_min 1: every level has a lookup order), counts and checksums printed for the parent to compare."""
    import tempfile
    rng = np.random.default_rng(11)
    text = "\n".join(pile(rng, "T", 60, 10000, 14000, ["Q0", "Q1", "Q2", "Q3"])) + "\n"
    with tempfile.TemporaryDirectory() as d:
        g, c = build_index(d, text)
        fused_options(g)
        ranges = covering(g, "T", 200, 9000, 16000, 3)
        out = []
        for kw in ({}, dict(M1, max_depth=2), dict(M1, max_depth=3)):
            check_forms(g, c, ranges, kw, forms=FORMS, cache={}, tag=("lib sort", os.environ.get("IMPG_LIB_SORT")))
            st, cnt, ck = g.query_batch_stats(ranges, impg_amd.make_params(**kw))
            out.append((int(st.projected), int(cnt.sum()), int(np.bitwise_xor.reduce(ck))))
        print("LIB_SORT_RESULT %r" % (out,), flush=True)


def test_library_sort_in_a_fresh_process():
    """IMPG_LIB_SORT is read once per process: a child with it set and one without, the same batch, the same answers (each
    also checked against the oracle in the child)."""
    got = []
    for val in ("1", None):
        env = dict(os.environ)
        env.pop("IMPG_LIB_SORT", None)
        if val:
            env["IMPG_LIB_SORT"] = val
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "lib_sort_child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (val, r.stdout[-2000:], r.stderr[-4000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LIB_SORT_RESULT ")]
        assert len(lines) == 1, r.stdout[-2000:]
        got.append(lines[0])
    assert got[0] == got[1]


if __name__ == "__main__":
    assert sys.argv[1:] == ["lib_sort_child"]
    lib_sort_child()
