"""`impg partition` on the host twin (impg_gpu_regions_* with on_host = 1; no GPU): the region algebra against the
sequential restatement of tests/partition_ref.py after every window, the selection modes, the window rules, rehoming
and the text writers."""
import numpy as np
import pytest

import impg_amd
from impg_amd import _lib
from tests import partition_ref as pr


def check_steps(windows, lens, d, mm, mb, on_host=True, ref=None, reg=None):
    ref = ref or pr.Ref(lens)
    reg = reg or impg_amd.Regions(lens, on_host=on_host)
    for k, rows in enumerate(windows):
        want = ref.apply(rows, d, mm, mb)
        got = reg.apply(pr.rows_array(rows), d, mm, mb)
        assert got == want, (k, rows[:8])
        assert reg.get("masked") == ref.masked.table(), k
        assert reg.get("missing") == ref.missing.table(), k
    return ref, reg


CASES = ["reverse", "duplicate", "end_dist_199", "end_dist_200", "end_dist_201", "frag_299", "frag_300", "frag_301", "equal_mask",
         "inside_mask", "both_to_zero", "touching", "emptied_missing"]


def test_random_sequence_of_windows():
    windows = pr.scripted_windows() + pr.random_windows(np.random.default_rng(5), pr.LENS, 40 - len(pr.scripted_windows()))
    assert len(windows) == 40
    ref, _ = check_steps(windows, pr.LENS, 100, 300, 200)
    assert [c for c in CASES if c not in ref.seen] == []
    assert ref.count["extensions"] > 0 and ref.count["splits"] > 0 and ref.count["empty_windows"] > 0
    assert ref.count["boundary_extensions"] > 0


def test_merge_distance_zero():
    ref, _ = check_steps(pr.scripted_windows() + pr.random_windows(np.random.default_rng(6), pr.LENS, 10), pr.LENS, 0, 300, 200)
    assert ref.count["extensions"] > 0 and ref.count["splits"] > 0


def test_no_boundary_extension():
    ref, _ = check_steps(pr.scripted_windows() + pr.random_windows(np.random.default_rng(7), pr.LENS, 10), pr.LENS, 100, 300, 0)
    assert ref.count["boundary_extensions"] == 0 and ref.count["extensions"] > 0


def test_negative_merge_distance_is_refused():
    reg = impg_amd.Regions(pr.LENS, on_host=True)
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        reg.apply(pr.rows_array([(0, 1, 2)]), -1)
    assert e.value.code == impg_amd.IMPG_E_INVALID


NAMES = ["A#1#chr1", "A#1#chr2", "A#2#chr1", "B#1#chr1", "B#1#chr2", "C#1#chr1"]


def test_select_modes():
    lens = [30000, 30000, 45000, 40000, 15000, 10000]
    # seq 0 keeps (0, 10000) and (20000, 30000): an equal-length tie inside a sequence; seq 1 keeps (0, 5000), (15000, 30000)
    windows = [[(0, 10000, 20000)], [(1, 5000, 15000)], [(2, 0, 45000)], [(3, 0, 30000)]]
    ref, reg = check_steps(windows, lens, 0, 0, 0)
    for mode in ("longest", "total", "sample", "haplotype", "haplotype,#", "sample,#"):
        for w in (4000, 7000, 100000):
            assert reg.select(mode, w, NAMES) == ref.select(mode, w, NAMES), (mode, w)
    # missing range lengths: 10000, 10000 | 5000, 15000 | - | 10000 | 15000 | 10000
    assert reg.select("longest", 100000) == [(4, 0, 15000)]  # 15000 on 1 and on 4: the higher id wins
    assert reg.select("total", 100000) == [(1, 0, 30000)]    # 20000 missing bases on 0 and on 1: the higher id wins
    assert reg.select("sample", 100000, NAMES) == [(0, 0, 30000), (1, 0, 30000)]  # A: 40000 (seq 2 has left the map); equal lengths by id
    assert reg.select("haplotype,#", 100000, NAMES) == [(0, 0, 30000), (1, 0, 30000)]
    # the equal-length tie of `longest`: the later range of the higher sequence
    ref2, reg2 = check_steps([[(4, 0, 15000)], [(3, 30000, 40000)], [(5, 0, 10000)], [(1, 15000, 20000)]], lens, 0, 0, 0, ref=ref, reg=reg)
    assert ref2.select("longest", 100000) == [(1, 20000, 30000)]
    assert reg2.select("longest", 100000) == [(1, 20000, 30000)]
    assert reg2.select("longest", 4000) == [(1, 20000, 24000), (1, 24000, 30000)]  # the tail window joins its predecessor
    with pytest.raises(ValueError):
        reg.select("largest", 10)


def test_starting_window_tail_rules():
    lens = [10000, 2500, 9000]
    for ids in ([0, 1, 2], [1, 0], [2, 2], [1]):
        for w in (3000, 4000, 10000):
            assert impg_amd.starting_windows(ids, lens, w) == pr.starting_windows(ids, lens, w), (ids, w)
    # a short tail joins the previous window of the SAME sequence only: sequence 1 is shorter than a window and stays one
    assert impg_amd.starting_windows([0, 1], lens, 3000) == [(0, 0, 3000), (0, 3000, 6000), (0, 6000, 10000), (1, 0, 2500)]
    # select_and_window_sequences' rule is per range
    reg = impg_amd.Regions(lens, on_host=True)
    assert reg.select("total", 3000) == [(0, 0, 3000), (0, 3000, 6000), (0, 6000, 10000)]


PARTS = [(0, [(0, 0, 100), (1, 0, 50), (0, 300, 400)]),
         (1, [(0, 100, 200)]),          # singleton, left flank in partition 0: moves in pass 1
         (2, [(0, 200, 300)]),          # singleton between two singletons' worth of flanks: both flanks are non-singletons -> 0
         (3, [(1, 50, 80)]),            # singleton next to (1, 0, 50) of partition 0
         (4, [(1, 200, 300)]),          # singleton without flanks: stays
         (5, [(2, 0, 10), (2, 10, 20)]),
         (6, [(2, 20, 30)]),            # cascade: first of two singletons in a row, flank in 5
         (7, [(2, 30, 40)])]            # ... its neighbour is a singleton in pass 1 and a member of 5 in pass 2


def test_rehome_singleton_slivers():
    want, moved = pr.rehome_singleton_slivers([(p, list(iv)) for p, iv in PARTS])
    assert moved >= 5
    assert [p for p, _ in want] == [0, 4, 5]
    assert (2, 30, 40) in dict(want)[5]  # the second singleton of the cascade arrived
    assert impg_amd.rehome_singleton_slivers(PARTS) == want
    assert impg_amd.rehome_singleton_slivers([(0, [(0, 0, 5), (0, 9, 12)])]) == [(0, [(0, 0, 5), (0, 9, 12)])]


def test_bed_text_bytes():
    names = ["S#1#chr1", "S#1#chr2", "T#1#chr1"]
    assert impg_amd.partitions_bed_text(PARTS, names) == pr.bed_text(PARTS, names)
    assert impg_amd.partitions_bed_text([(3, [(1, 5, 9)])], names) == "S#1#chr2\t5\t9\t3\n"
    assert impg_amd.partitions_bed_text([], names) == ""


def test_rows_beyond_the_callers_buffer_are_kept():
    import ctypes as C
    ref = pr.Ref(pr.LENS)
    rows = [(0, 100 + 1000 * k, 600 + 1000 * k) for k in range(12)] + [(3, 5000, 5100)]
    want = ref.apply(rows, 100, 300, 0)
    assert len(want) == 13
    reg = impg_amd.Regions(pr.LENS, on_host=True)
    a = pr.rows_array(rows)
    small = np.zeros(2, dtype=_lib.PARTITION_ROW_DTYPE)
    n = C.c_size_t(0)
    _lib.check(_lib.lib().impg_gpu_regions_apply(reg._h, a.ctypes.data, a.size, 100, 300, 0, small.ctypes.data, 2, C.byref(n)))
    assert n.value == 13 and [tuple(int(x) for x in r) for r in small] == want[:2]
    assert reg._rows(small, n.value) == want               # fetched whole; the state moved on once
    assert reg.get("masked") == ref.masked.table() and reg.get("missing") == ref.missing.table()


# ---- small, collision-dense universes (the inputs of tests/test_gpu_partition_algebra.py, proven here without a GPU) ----
DENSE_SEEDS = range(150)


@pytest.mark.parametrize("variant", list(pr.DENSE_VARIANTS))
def test_dense_universes(variant):
    """check_steps' comparison plus the selections, after each of 12 windows of 150 seeds; what the seeds must have
    reached is asserted from the restatement alone, before the twin is looked at."""
    cases, reached = pr.dense_reference(DENSE_SEEDS, **pr.DENSE_VARIANTS[variant])
    want = pr.DENSE_REACH + ([pr.ZERO_LEN_REACH] if variant == "zero_len" else [])
    assert [c for c in want if c not in reached] == []
    for seed, lens, w, steps in cases:
        pr.replay(impg_amd.Regions(lens, on_host=True), steps, w)


@pytest.mark.parametrize("n_seq", [1, 2, 255, 256, 257, 1024])
def test_sparse_universes(n_seq):
    lens, params, windows = pr.sparse_case(n_seq)
    assert n_seq < 4 or lens.count(0) >= 1
    pr.replay(impg_amd.Regions(lens, on_host=True), pr.ref_steps(pr.Ref(lens), windows, params, max(lens)), max(lens))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_row_counts(n):
    lens, windows = pr.row_count_case(n)
    ref = pr.Ref(lens)
    steps = [st for rows, params in windows for st in pr.ref_steps(ref, [rows], params, lens[0])]
    assert [len(st[2]) for st in steps] == [n, n, n, 0]  # fresh, each split by the mask, each extended, each swallowed
    assert ref.count["extensions"] == 2 * n - min(n, 2)  # (the last interval of a sequence is far from its end)
    pr.replay(impg_amd.Regions(lens, on_host=True), steps, lens[0])


def test_piece_counts_and_clamped_length():
    lens, params, windows = pr.piece_count_case()
    steps = pr.ref_steps(pr.Ref(lens), [rows for rows, _ in windows], params, 100)
    assert [len(st[2]) for st in steps] == [pieces for _, pieces in windows]
    pr.replay(impg_amd.Regions(lens, on_host=True), steps, 100)
    given, kept, params, windows = pr.clamp_case()
    reg = impg_amd.Regions(given, on_host=True)
    assert reg.get("missing")[0] == [(0, pr.I32_MAX)]
    pr.replay(reg, pr.ref_steps(pr.Ref(kept), windows, params, pr.I32_MAX), pr.I32_MAX)


def test_dense_ties():
    lens, params, windows = pr.tie_case()
    modes = ("longest", "total", "sample", "haplotype")
    for w in (1000, 300):
        pr.replay(impg_amd.Regions(lens, on_host=True), pr.ref_steps(pr.Ref(lens), windows, params, w, pr.TIE_NAMES, modes), w, pr.TIE_NAMES)
