"""tests/prims_gen.py is what tests/test_gpu_prims.py assumes it is (no GPU): the scans' inputs keep the kernels' stated
precondition while their totals pass 2^32, the huge lengths pass 2^32 where the test says, and the key sort's reference
is the lexicographic order."""
import numpy as np

import impg_amd
from tests import prims_gen as pg


def block_sums(a, tile):
    padded = np.zeros((len(a) + tile - 1) // tile * tile, dtype=np.uint64)
    padded[:len(a)] = a
    return padded.reshape(-1, tile).sum(axis=1)


def test_heavy_keeps_every_tile_sum_below_2_32_and_its_total_above():
    """the kernels' precondition is on the inputs, for both tilings; the total is what must pass 2^32"""
    used = 0
    for sizes in (pg.LOOKBACK_SIZES, pg.THREE_KERNEL_SIZES):
        assert pg.scan_patterns(sizes[-1], sizes) == pg.scan_patterns(sizes[-2], sizes) == ["small", "heavy"]
        for n in sizes:
            pats = pg.scan_patterns(n, sizes)
            assert ("heavy" in pats) == (n > 2 * 4096), n
            if n not in sizes[-2:]:
                assert set(pats) >= set(pg.SCAN_PATTERNS) - {"heavy"}
            if "heavy" not in pats:
                continue
            used += 1
            a = pg.scan_input("heavy", n)
            assert a.dtype == np.uint32 and len(a) == n and not a.flags.writeable
            for tile in (2048, 4096):
                assert int(block_sums(a, tile).max()) < 1 << 32, (n, tile)
            assert int(a.astype(np.uint64).sum()) >= 1 << 32, n
            heavy = np.flatnonzero(a > 1)
            assert heavy.tolist() == list(range(0, n, 8192)) and (a[heavy] == 1 << 31).all()
            want, total = pg.scan_reference("heavy", n)
            assert total == sum(int(x) for x in a[heavy]) + int((a == 1).sum())
            assert int(want[8192]) == int(a[:8192].astype(np.uint64).sum()) & 0xFFFFFFFF
    assert used >= 12


def test_the_other_patterns_and_the_size_lists():
    assert (pg.LB_TILE, pg.SCAN_TILE) == (4096, 2048)
    assert {64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1, 65 * 4096 + 17, 4080, 16} <= set(pg.LOOKBACK_SIZES)
    assert {1024 * 2048 - 1, 1024 * 2048, 1024 * 2048 + 1, 1025 * 2048 + 3, 2049 * 2048 + 1, 1023 * 2048 + 5} <= set(pg.THREE_KERNEL_SIZES)
    for n in (1, 17, 4097):
        assert pg.scan_input("zeros", n).sum() == 0 and pg.scan_input("ones", n).sum() == n
        first, last = pg.scan_input("first", n), pg.scan_input("last", n)
        assert first[0] == 7 and last[n - 1] == 7 and first.sum() == last.sum() == 7
        assert pg.scan_input("small", n).max() <= 3
    want, total = pg.scan_reference("ones", 4097)
    assert want.tolist() == list(range(4097)) and total == 4097
    for n in pg.SMALL_SCAN_SIZES:
        for p in pg.SMALL_SCAN_PATTERNS:
            assert pg.scan_reference(p, n)[1] < 1 << 32


def test_huge_lengths_pass_2_32_at_item_2():
    for n in pg.OFFSET_SIZES:
        text, huge = pg.lengths("text", n), pg.lengths("huge", n)
        assert text.min() >= 20 and text.max() <= 200
        assert np.flatnonzero(huge != text).tolist() == sorted({0, min(1, n - 1), n - 1})
        prefix, total = pg.exclusive_prefix(huge)
        assert prefix[0] == 0 and (n < 2 or prefix[1] == 0xF0000000)
        if n >= 2:
            assert total >= 1 << 32
        if n >= 3:
            assert int(prefix[2]) == 2 * 0xF0000000 >= 1 << 32 and (prefix[2:] >= 1 << 32).all()
        assert total == sum(int(x) for x in huge)


def test_sort_reference_is_the_lexicographic_order():
    """shape (b): perm is the identity, so pass by pass, least significant first, is np.lexsort on the masked keys"""
    for shape in ("b", "b64"):
        for m in pg.SORT_SIZES:
            for noise in (False, True):
                n_keys, perm, passes, first_in_order = pg.sort_case(shape, m, noise)
                assert first_in_order and n_keys == m and perm.tolist() == list(range(m))
                (k32, b32), (k64, b64) = passes
                assert k32.dtype == np.uint32 and k64.dtype == np.uint64
                want = np.lexsort((pg.key_mask(k32, b32), pg.key_mask(k64, b64)))
                assert pg.sort_reference(perm, passes).tolist() == want.tolist(), (shape, m, noise)


def test_sort_cases_have_ties_noise_and_dropped_rows():
    for shape, (spec, first_in_order, drops) in pg.SORT_SHAPES.items():
        for m in pg.SORT_SIZES:
            plain, noisy = pg.sort_case(shape, m, False), pg.sort_case(shape, m, True)
            n_keys, perm = plain[0], plain[1]
            assert len(perm) == m and n_keys == (m + m // 5 if drops else m)
            if drops:
                assert set(range(n_keys)) - set(perm.tolist()) == set(range(5, n_keys, 6))
            for (keys, bits), (nkeys, _), (wide, sbits) in zip(plain[2], noisy[2], spec):
                assert bits == sbits and keys.dtype == (np.uint64 if wide else np.uint32) and len(keys) == n_keys
                assert len(np.unique(pg.key_mask(keys, bits))) <= 5 and len(np.unique(pg.key_mask(nkeys, bits))) <= 5
                assert (pg.key_mask(keys, bits) == keys).all()
                if m >= 255 and bits < (64 if wide else 32):
                    assert (pg.key_mask(nkeys, bits) != nkeys).any()  # bits above `bits` are set ...
                    assert len(np.unique(nkeys)) > 5                  # ... and would change the order if they counted
    assert pg.SORT_SHAPES["a"][0] == [(False, 32), (True, 33 + pg.SEQ_BITS), (True, pg.RANGE_BITS + pg.SEQ_BITS)]
    assert pg.SORT_SHAPES["c"][0] == [(False, 3)]


def test_python_entry_points_exist():
    from impg_amd import _lib, index
    assert {"impg_gpu_selftest_scan", "impg_gpu_selftest_offsets", "impg_gpu_selftest_key_sort"} <= {n for n, _, _ in _lib.SYMBOLS}
    assert callable(index.selftest_scan) and callable(index.selftest_offsets) and callable(index.selftest_key_sort)
    assert impg_amd.lib() is not None
