"""project_entries_kernel's scan -- which of a block's ranges hit the entry a wave holds -- at its edges, against the oracle.

The kernel pads the windows of a level's last block with empty ones and tests whole groups of 64 ranges; a block without a
window wider than the 64-bit hit mask takes a scan that reads nothing but the mask bit (the narrow variant), any other
block the general one with the wide windows' test on the entry's own end.  Every case here runs the counting form
(`stats`, OUT_SLOTS) and the attributed rows (`attributed`, OUT_QS), plain and `-x -m 1`, compares per-range counts,
checksums and rows with the oracle and asserts that the entries kernel ran the level.

What the lookup's windows allow (lookup_count_lane_kernel): a window starts at the first entry whose running maximum of
ends reaches the range's start, and that entry's own end is the maximum there -- bit 0 of a non-empty window is always
set, so neither "the only hit is bit 63" nor "a non-empty window with no mask bit" can be built from a PAF.  The mask
cases below therefore keep bit 0 and make bit 31, 32 or the window's last bit the only OTHER hit, with up to 62 misses in
between, and put ranges whose window is empty (no entry of the target near them) between the hitting ones.  A window
whose start is no multiple of 4 is narrow only up to 64 - (start mod 4) entries: the last bit tested is 63, 62, 61 and 60
for the four residues."""
import numpy as np
import pytest

import impg_amd
from tests.paf_gen import spans
from tests.proj_worker import build_index, check_forms
from tests.test_gpu_projection_paths import ENT_QS, ENT_RANGES, ENT_SLOTS, L, M1, covering, fused_options, pile

pytestmark = pytest.mark.gpu

FORMS = ("stats", "attributed")


def check_entries(g, c, ranges, cache, tag, x1=M1):
    """Both forms, plain and -x -m 1, against the oracle; the entries kernel must have run each of them."""
    for kw in ({}, x1):
        arms = check_forms(g, c, ranges, kw, forms=FORMS, cache=cache, expect=dict(stats=ENT_SLOTS), tag=tag)
        a = arms["attributed"]
        assert a.get(ENT_QS, 0) > 0 or a.get(ENT_SLOTS, 0) > 0, (tag, kw, a)
        if not kw:  # (a plain call keeps the fused level as {query id, place} pairs)
            assert a.get(ENT_QS, 0) > 0, (tag, a)


# ---- padded ranges: the level's last block holds 32 .. 511 ranges, or one --------------------------------------------------
@pytest.fixture(scope="module")
def pile40(tmp_path_factory):
    """40 records on T (one direction: 40 index entries), 1 025 ranges that each cover all of them, and one cache of the
    oracle's answers for every case (the cases take prefixes of the same list)."""
    rng = np.random.default_rng(7)
    text = "\n".join(pile(rng, "T", 40, 10000, 12000, ["Q%d" % i for i in range(8)])) + "\n"
    g, c = build_index(str(tmp_path_factory.mktemp("scan40")), text, bidirectional=False)
    assert g.num_entries() == 40
    return g, c, covering(g, "T", 1025, 9000, 15000, 1025), {}


@pytest.mark.parametrize("n", [32, 63, 64, 65, 511, 512, 513, 1025])
def test_padded_last_block(pile40, n):
    """n ranges, 40 pairs each: n pairs per entry (32 is the fused threshold).  The last block has n mod 512 ranges -- 32, 63,
    64, 65, 511, a full 512, and one range alone in a second / third block; the windows behind them are padding that must
    never hit (a hit would write a place beyond the block's and change counts and checksums)."""
    g, c, ranges, cache = pile40
    fused_options(g)
    st, _, _ = g.query_batch_stats(ranges[:n], impg_amd.make_params(), counts=False, checksums=False)
    assert st.pairs == 40 * n
    check_entries(g, c, ranges[:n], cache, ("padded", n))


# ---- mask edges -----------------------------------------------------------------------------------------------------------------
def _line(q, strand, ts, ops, qs=1000):
    td, qd = spans(ops)
    cg = "".join("%d%s" % (ln, c) for ln, c in ops)
    return "%s\t%d\t%d\t%d\t%s\tT\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%s" % (q, L, qs, qs + qd, strand, L, ts, ts + td, td, td + qd, cg)


SHORT = [(10, "="), (2, "X"), (3, "I"), (4, "D"), (8, "=")]          # 24 bp of target
MID31 = [(50, "="), (1, "X"), (2, "I"), (3, "D")] * 5 + [(30, "=")]  # 300 bp
MID32 = MID31 + [(40, "=")]                                          # 340 bp
RIGHT = [(50, "="), (1, "X"), (2, "I"), (3, "D")] * 9 + [(14, "=")]  # 500 bp
LONG = [(50, "="), (1, "X"), (2, "I"), (3, "D")] * 30                # 1 620 bp, 120 ops
assert [spans(o)[0] for o in (SHORT, MID31, MID32, RIGHT, LONG)] == [24, 300, 340, 500, 1620]
BASES = [10000 + 100000 * j for j in range(4)]


@pytest.fixture(scope="module")
def edge_index(tmp_path_factory):
    """Four groups of records along T, group j at B = BASES[j], its entries consecutive in the index (sorted by start):
      fillers (4, 1, 2, 3 of them: the group's first real entry sits at index = j mod 4), far below B
      LONG   at B, ends B + 1620                                  -- bit 0 of every window of the group
      SHORT  at B + 4 k for k = 1 .. 62 - j, 24 bp (all end by B + 272), but
      MID31  at k = 31, ends B + 424, and MID32 at k = 32, ends B + 468   -- bits 31 and 32
      RIGHT  at B + 500, ends B + 1000                            -- bit 63 - j, the last one a narrow window at that start can hold"""
    lines, idx, first = [], 0, []
    for j, B in enumerate(BASES):
        n_fill = 4 if j == 0 else j
        for f in range(n_fill):
            lines.append(_line("Q%d" % (f % 4), "+-"[f % 2], B - 900 + 100 * f, SHORT, qs=2000 + 50 * f))
        idx += n_fill
        first.append(idx)
        lines.append(_line("Q0", "+", B, LONG, qs=5000))
        for k in range(1, 63 - j):
            ops = MID31 if k == 31 else MID32 if k == 32 else SHORT
            lines.append(_line("Q%d" % (k % 4), "+-"[k % 2], B + 4 * k, ops, qs=10000 + 400 * k))
        lines.append(_line("Q1", "-", B + 500, RIGHT, qs=50000))
        idx += 64 - j
    assert [f % 4 for f in first] == [0, 1, 2, 3]
    g, c = build_index(str(tmp_path_factory.mktemp("scanedge")), "\n".join(lines) + "\n", bidirectional=False)
    assert g.num_entries() == idx
    return g, c


def test_mask_edge_bits(edge_index):
    """Per group: ranges whose hits are bit 0 alone (a window of 64 - j entries, 63 - j misses behind the hit), bits 0 and 31,
    0 and 32 (at MID31's very end: the plain and the transitive end test differ by that one base), 0, 31 and 32, and bit 0
    with the window's last bit; ranges with an empty window between them; and 60 ranges over most of the group, which make
    the level dense enough to be fused."""
    g, c = edge_index
    fused_options(g)
    T = g.seq_id("T")
    rng = np.random.default_rng(3)
    ranges = []
    for B in BASES:
        edges = [(B + 1100, B + 1200),  # LONG only; the window runs to RIGHT: bit 0 of 64 - j
                 (B + 1001, B + 1002),
                 (B + 600, B + 700),    # LONG and RIGHT: bit 0 and the last bit
                 (B + 999, B + 1000), (B + 1000, B + 1001),  # RIGHT's last base, and one past it (plain: end >= start still hits)
                 (B + 469, B + 499),    # LONG only, the window ends before RIGHT: bit 0 of 63 - j
                 (B + 430, B + 440),    # LONG and MID32: bits 0, 32
                 (B + 424, B + 428),    # MID31 ends here: bits 0, 31 (plain only), 32
                 (B + 400, B + 410),    # bits 0, 31, 32
                 (B + 468, B + 469),    # MID32 ends here
                 (B + 280, B + 290)]    # past every SHORT: bits 0, 31, 32
        empty = [(B - 300, B - 200), (B + 1700, B + 1800), (B + 5000, B + 5100)]  # no entry there: lo == ub
        bulk = [(B + int(rng.integers(90, 110)), B + int(rng.integers(1000, 3000))) for _ in range(60)]
        for k, e in enumerate(edges):  # (an empty window between two hitting ranges, and the bulk around them)
            ranges += [(T,) + e, (T,) + empty[k % 3], (T,) + bulk[k]]
        ranges += [(T,) + b for b in bulk[len(edges):]]
    st, _, _ = g.query_batch_stats(ranges, impg_amd.make_params(), counts=False, checksums=False)
    assert st.pairs >= 32 * g.num_entries() and len(ranges) <= ENT_RANGES, (st.pairs, g.num_entries(), len(ranges))
    # (-x -m 1 with min_transitive_len 1: the one-base ranges at the records' ends stay in)
    check_entries(g, c, ranges, {}, "mask edges", x1=dict(M1, min_transitive_len=1))


# ---- the variant a block takes --------------------------------------------------------------------------------------------------
def test_wide_window_among_narrow(tmp_path):
    """600 ranges over a 40-entry pile (narrow windows: two blocks in the lookup order) and ONE range over a pile of 100
    records on another target, whose window is wider than the mask: the block it lands in takes the general scan, the other
    the narrow one, in the same launch.  Under -x the wide window's test is the transitive one (an end equal to the range's
    start does not hit)."""
    rng = np.random.default_rng(19)
    lines = pile(rng, "T", 40, 10000, 12000, ["Q%d" % i for i in range(8)])
    lines += pile(rng, "W", 100, 10000, 10400, ["Q%d" % i for i in range(8)], min_ops=2, max_ops=8)
    g, c = build_index(str(tmp_path), "\n".join(lines) + "\n", bidirectional=False)
    assert g.num_entries() == 140
    fused_options(g)
    W = g.seq_id("W")
    wide = (W, 9000, 12000)
    narrow = covering(g, "T", 600, 9000, 15000, 600)
    cache = {}
    ranges = narrow[:300] + [wide] + narrow[300:]
    st, _, _ = g.query_batch_stats(ranges, impg_amd.make_params(), counts=False, checksums=False)
    assert st.pairs == 600 * 40 + 100
    check_entries(g, c, ranges, cache, "wide among narrow")
    # (the wide window alone in its block's company: every hit of the block through the general scan, ends at the range's start included)
    ends = [(W, 10000 + k, 10000 + k + 1) for k in range(0, 400, 7)]
    check_entries(g, c, narrow[:200] + ends + [wide], cache, "wide, one-base ranges")


# ---- the orientations ------------------------------------------------------------------------------------------------------------
def test_orientations_in_one_block(tmp_path):
    """One block of 460 ranges whose entries are forward (the pile on U from its target side), reversed on either strand (the
    same records from their query sides: a bidirectional index) and, every 4th, a record of 260 ops -- more than the 208 a
    staged record holds (ORIENT = -1, from the index)."""
    rng = np.random.default_rng(23)
    text = "\n".join(pile(rng, "U", 24, 10000, 11000, ["Q0", "Q1", "Q2", "Q3"], min_ops=20, max_ops=50, long_ops=260, long_every=4)) + "\n"
    g, c = build_index(str(tmp_path), text)
    assert g.num_entries() == 48
    fused_options(g)
    U = g.seq_id("U")
    ranges = [(U, int(rng.integers(5000, 10000)), int(rng.integers(11000, 30000))) for _ in range(300)]
    for q in range(4):
        qid = g.seq_id("Q%d" % q)
        ranges += [(qid, int(rng.integers(0, L // 2)), int(rng.integers(L // 2, L))) for _ in range(40)]
    assert len(ranges) <= ENT_RANGES
    st, _, _ = g.query_batch_stats(ranges, impg_amd.make_params(), counts=False, checksums=False)
    assert st.pairs >= 32 * g.num_entries()
    check_entries(g, c, ranges, {}, "orientations")
