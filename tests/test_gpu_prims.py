"""The device primitives every stage stands on, on their own (impg_amd/csrc/prims_selftest.hip): the exclusive scan behind
Engine::scan / scan2 in both of its forms, the small-batch path's single-block scan, the 64-bit offsets of a list of
lengths (rocPRIM, uint32 -> uint64) and the stable multi-key sort that orders the rows of BED, BEDPE, PAF and FASTA.  The
inputs are tests/prims_gen.py's, the reference is numpy in uint64; an entry returns the device's raw answer and the
comparison happens here.  No engine, no index, every case small."""
import numpy as np
import pytest

from impg_amd import index as ix
from tests import prims_gen as pg

pytestmark = pytest.mark.gpu

LOOKBACK_SHIFTS = [(0, 0), (4, 0), (0, 4)]      # (in, out) words behind a 256-byte boundary: 4 words = aligned again
THREE_KERNEL_SHIFTS = [(1, 0), (0, 2), (3, 3)]


def check_scan(pattern, n, shifts, form):
    """one scan of scan_input(pattern, n): the form that ran, the form's rule, every offset and the total"""
    want, want_total = pg.scan_reference(pattern, n)
    out, total, info = ix.selftest_scan(pg.scan_input(pattern, n), 0, *shifts)
    what = (pattern, n, shifts)
    assert (info["lookback_tile"], info["three_kernel_tile"]) == (pg.LB_TILE, pg.SCAN_TILE), info
    assert (info["form"] == ix.SCAN_LOOKBACK) == (info["in_low4"] == 0 and info["out_low4"] == 0), (what, info)
    assert info["form"] == form, (what, info)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, (what, "first wrong offset at", int(bad[0]), int(out[bad[0]]), int(want[bad[0]]), "of", bad.size)
    assert total == want_total, (what, total, want_total)


def test_scan_form_follows_alignment():
    """The look-back form runs if and only if both device addresses are multiples of 16, both forms ran, and the tile
    sizes are the ones prims_gen's size lists are built from (a retune must fail here, not silently move the edges)."""
    forms = set()
    for shifts in LOOKBACK_SHIFTS + THREE_KERNEL_SHIFTS:
        _, _, info = ix.selftest_scan(pg.scan_input("small", 12301), 0, *shifts)
        assert (info["lookback_tile"], info["three_kernel_tile"]) == (4096, 2048)
        assert (info["in_low4"], info["out_low4"]) == (4 * shifts[0] % 16, 4 * shifts[1] % 16), (shifts, info)
        aligned = info["in_low4"] == 0 and info["out_low4"] == 0
        assert aligned == (shifts in LOOKBACK_SHIFTS)
        assert info["form"] == (ix.SCAN_LOOKBACK if aligned else ix.SCAN_THREE_KERNEL), (shifts, info)
        forms.add(info["form"])
    assert forms == {ix.SCAN_LOOKBACK, ix.SCAN_THREE_KERNEL}


@pytest.mark.parametrize("n", pg.LOOKBACK_SIZES)
def test_scan_lookback(n):
    """The single-pass look-back kernel at its edges: one thread's 16 items (the uint4 path) and the scalar path of a
    partial last tile, the last thread's border, one tile and the next, the 64-tile look-back window and past it; totals
    beyond 2^32 (heavy: the offsets are the prefixes' low 32 bits, the total exact); nothing written outside out[0 .. n)
    or past scan_scratch_bytes(n) (the entry's guards).  The look-back's second window (`j -= 64`: none of the 64 nearest
    tiles has its inclusive prefix yet) is reached only by timing and is NOT forced here: with more than 64 tiles it may
    or may not run."""
    for pattern in pg.scan_patterns(n, pg.LOOKBACK_SIZES):
        for shifts in LOOKBACK_SHIFTS:
            check_scan(pattern, n, shifts, ix.SCAN_LOOKBACK)


@pytest.mark.parametrize("n", pg.THREE_KERNEL_SIZES)
def test_scan_three_kernels(n):
    """scan_block_sums / scan_of_sums / scan_apply, the form of a pointer that is not 16-byte aligned: one thread's 8
    items, one block and the next, 1 024 block sums (the last size with one sum per scan_of_sums thread), 1 025 (two per
    thread, idle threads) and 2 050 (three); totals beyond 2^32; the guards as above."""
    for pattern in pg.scan_patterns(n, pg.THREE_KERNEL_SIZES):
        for shifts in THREE_KERNEL_SHIFTS:
            check_scan(pattern, n, shifts, ix.SCAN_THREE_KERNEL)


@pytest.mark.parametrize("n", pg.SMALL_SCAN_SIZES)
def test_small_scan(n):
    """small_scan_kernel, the single block of the small-batch path (n <= 1 024): offsets and the exact 32-bit total"""
    for pattern in pg.SMALL_SCAN_PATTERNS:
        want, want_total = pg.scan_reference(pattern, n)
        assert want_total < 1 << 32
        for shifts in [(0, 0), (1, 3)]:
            out, total, info = ix.selftest_scan(pg.scan_input(pattern, n), 1, *shifts)
            assert info["form"] == ix.SCAN_SMALL
            assert out.tolist() == want.tolist(), (pattern, n, shifts)
            assert total == want_total, (pattern, n, shifts)


def test_scan_refuses_what_it_cannot_run():
    for kw in (dict(which=2), dict(which=1, n=1025), dict(in_shift=5), dict(out_shift=5), dict(n=0)):
        with pytest.raises(ix.ImpgGpuError) as e:
            ix.selftest_scan(np.ones(kw.pop("n", 8), dtype=np.uint32), **kw)
        assert e.value.code == ix._lib.IMPG_E_INVALID


@pytest.mark.parametrize("pattern", pg.OFFSET_PATTERNS)
def test_offsets_are_64_bit(pattern):
    """prims::offsets_and_total (rocPRIM's exclusive scan from uint32 lengths into uint64 offsets): every offset and the
    total exact in 64 bits -- with `huge` the sum passes 2^32 from the second item on --, with and without the host copy
    of the offsets (the two read the total differently)."""
    for n in pg.OFFSET_SIZES:
        a = pg.lengths(pattern, n)
        want, want_total = pg.exclusive_prefix(a)
        for with_host_copy in (False, True):
            off, total = ix.selftest_offsets(a, with_host_copy)
            assert off.dtype == np.uint64 and np.array_equal(off, want), (pattern, n, with_host_copy)
            assert total == want_total, (pattern, n, with_host_copy, total, want_total)


@pytest.mark.parametrize("shape", sorted(pg.SORT_SHAPES))
def test_key_sort(shape):
    """prims::KeySort::run as its callers shape it -- a: three gathering passes over the kept rows of a larger set; b, b64:
    the first pass in place, then a wide one; c: one narrow pass.  The keys stand at the rows' own indices, the order is a
    permutation of the kept rows, stable pass by pass with the least significant first, only the low `bits` bits of a key
    count (noise: random bits above them), and sorted_keys holds the last pass's keys in that order."""
    for m in pg.SORT_SIZES:
        for noise in (False, True):
            n_keys, perm, passes, first_in_order = pg.sort_case(shape, m, noise)
            order, sorted_keys = ix.selftest_key_sort(n_keys, perm, passes, first_in_order)
            want = pg.sort_reference(perm, passes)
            bad = np.flatnonzero(order != want)
            assert bad.size == 0, (shape, m, noise, "first wrong place", int(bad[0]), int(order[bad[0]]), int(want[bad[0]]))
            last = passes[-1][0]
            assert sorted_keys.dtype == last.dtype and np.array_equal(sorted_keys, last[order]), (shape, m, noise)


def test_key_sort_refuses_rows_out_of_range():
    keys = np.zeros(4, dtype=np.uint32)
    for perm, first in (([0, 4], False), ([1, 0, 2, 3], True), ([0, 1], True)):
        with pytest.raises(ix.ImpgGpuError) as e:
            ix.selftest_key_sort(4, perm, [(keys, 8)], first)
        assert e.value.code == ix._lib.IMPG_E_INVALID
