"""Inputs and numpy references for the device primitives' tests (tests/test_gpu_prims.py; checked on their own, without a
GPU, by tests/test_prims_gen_cpu.py): the scans' sizes and count patterns, the lengths of the 64-bit offsets, and the key
sort's keys with their reference order.  Everything is a pure function of its arguments and cached: a test takes the
arrays read-only."""
import functools

import numpy as np

# the tile sizes the size lists are built from: the look-back kernel's (LB_TILE) and the three kernels' (SCAN_TILE).  The
# GPU test asserts that the library reports the same two, so that a retune fails there instead of moving the edges.
LB_TILE, SCAN_TILE = 4096, 2048
LB_ITEMS, LB_WINDOW = 16, 64  # one thread's items; the tiles one look-back step reads
SUMS_BLOCK = 1024             # scan_of_sums' threads: up to here one block sum per thread

# 16: one thread's items; 4 080: where the last thread's items start; 64 tiles: the look-back window
LOOKBACK_SIZES = [1, 2, 15, 16, 17, 4079, 4080, 4081, 4095, 4096, 4097, 8191, 8192, 8193, 12301, LB_WINDOW * LB_TILE - 1,
                  LB_WINDOW * LB_TILE, LB_WINDOW * LB_TILE + 1, (LB_WINDOW + 1) * LB_TILE + 17, 1_000_003]
# 1 024 block sums: the last size with one sum per scan_of_sums thread; 1 025: two per thread and idle threads; 2 050: three
THREE_KERNEL_SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 4097, 1023 * SCAN_TILE + 5, SUMS_BLOCK * SCAN_TILE - 1, SUMS_BLOCK * SCAN_TILE,
                      SUMS_BLOCK * SCAN_TILE + 1, 1025 * SCAN_TILE + 3, 2049 * SCAN_TILE + 1]
SMALL_SCAN_SIZES = [1, 2, 63, 64, 65, 1023, 1024]
SMALL_SCAN_PATTERNS = ["ones", "small", "last"]
assert LOOKBACK_SIZES[3] == LB_ITEMS and LOOKBACK_SIZES[6] == LB_TILE - LB_ITEMS and LOOKBACK_SIZES == sorted(LOOKBACK_SIZES)
assert THREE_KERNEL_SIZES == sorted(THREE_KERNEL_SIZES) and THREE_KERNEL_SIZES[-1] == 2049 * 2048 + 1

SCAN_PATTERNS = ["zeros", "ones", "small", "first", "last", "heavy"]
HEAVY_VALUE, HEAVY_STRIDE = 1 << 31, 2 * LB_TILE  # the first item of every second 4 096-aligned block
HEAVY_MIN_N = HEAVY_STRIDE + 1                    # three blocks and more: two heavy items, a total of 2^32 at least


def scan_patterns(n, sizes):
    """the patterns a scan test runs at size n of its list `sizes`: all of them (heavy from three blocks on), but at the
    two largest sizes only small and heavy"""
    if n in sizes[-2:]:
        return ["small", "heavy"]
    return [p for p in SCAN_PATTERNS if p != "heavy" or n >= HEAVY_MIN_N]


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=8)
def scan_input(pattern, n):
    """n counts (uint32) of a pattern.  Every aligned tile of either form sums below 2^32, the kernels' stated
    precondition; heavy's total passes 2^32."""
    rng = np.random.default_rng([n, SCAN_PATTERNS.index(pattern)])
    if pattern == "zeros":
        a = np.zeros(n, dtype=np.uint32)
    elif pattern == "ones":
        a = np.ones(n, dtype=np.uint32)
    elif pattern == "small":
        a = rng.integers(0, 4, n, dtype=np.uint32)
    elif pattern in ("first", "last"):
        a = np.zeros(n, dtype=np.uint32)
        a[0 if pattern == "first" else n - 1] = 7
    elif pattern == "heavy":
        if n < HEAVY_MIN_N:
            raise ValueError("heavy is for n of three blocks and more")
        a = rng.integers(0, 2, n, dtype=np.uint32)
        a[::HEAVY_STRIDE] = HEAVY_VALUE
    else:
        raise ValueError(pattern)
    return _frozen(a)


def exclusive_prefix(a):
    """(the exclusive prefix sums in uint64, the exact total as a Python int)"""
    inc = np.cumsum(a, dtype=np.uint64)
    prefix = np.empty(len(a), dtype=np.uint64)
    prefix[0] = 0
    prefix[1:] = inc[:-1]
    return prefix, int(inc[-1])


@functools.lru_cache(maxsize=8)
def scan_reference(pattern, n):
    """what a scan of scan_input(pattern, n) must write: (the low 32 bits of the 64-bit prefixes, the exact total)"""
    prefix, total = exclusive_prefix(scan_input(pattern, n))
    return _frozen((prefix & np.uint64(0xFFFFFFFF)).astype(np.uint32)), total


# ---- offsets ---------------------------------------------------------------------------------------------------------------
OFFSET_SIZES = [1, 2, 3, 256, 257, 70_001]
OFFSET_PATTERNS = ["text", "huge"]
HUGE_LEN = 0xF0000000


@functools.lru_cache(maxsize=None)
def lengths(pattern, n):
    """text: 20 .. 200 a row, like lines of text; huge: 0xF0000000 at items 0, 1 and n - 1 besides"""
    a = np.random.default_rng([n, 77]).integers(20, 201, n, dtype=np.uint32)
    if pattern == "huge":
        a[[0, min(1, n - 1), n - 1]] = HUGE_LEN
    elif pattern != "text":
        raise ValueError(pattern)
    return _frozen(a)


# ---- key sort --------------------------------------------------------------------------------------------------------------
SORT_SIZES = [1, 2, 3, 255, 256, 257, 4095, 4097, 100_003]
SEQ_BITS, RANGE_BITS = 3, 4
# per shape: (the passes' (wide, bits), least significant first; first_in_order; does perm drop rows)
SORT_SHAPES = {
    "a": ([(False, 32), (True, 33 + SEQ_BITS), (True, RANGE_BITS + SEQ_BITS)], False, True),  # BEDPE / PAF: every sixth row dropped
    "b": ([(False, 32), (True, 41)], True, False),
    "b64": ([(False, 32), (True, 64)], True, False),  # (a key that counts in full)
    "c": ([(False, 3)], True, False),
}


def sort_case(shape, m, noise):
    """-> (n_keys, perm, [(keys, bits)], first_in_order): m rows to sort; a pass's keys take at most five distinct values
    (their lowest and highest bit that counts set in some), so ties exist at every level; noise: random bits above `bits`,
    which must not matter."""
    spec, first_in_order, drops = SORT_SHAPES[shape]
    rng = np.random.default_rng([m, sorted(SORT_SHAPES).index(shape), int(noise)])
    n_keys = m + m // 5 if drops else m
    perm = np.arange(n_keys, dtype=np.uint32)
    if drops:
        perm = perm[perm % 6 != 5]
    assert len(perm) == m
    passes = []
    for wide, bits in spec:
        dt = np.uint64 if wide else np.uint32
        values = rng.integers(0, 1 << bits, 5, dtype=np.uint64, endpoint=False)
        values[0] |= np.uint64(1 << (bits - 1))
        values[1] = np.uint64(1)
        keys = values[rng.integers(0, 5, n_keys)]
        width = 64 if wide else 32
        if noise and bits < width:
            keys = keys | (rng.integers(0, 1 << (width - bits), n_keys, dtype=np.uint64) << np.uint64(bits))
        passes.append((_frozen(keys.astype(dt)), bits))
    return n_keys, _frozen(perm), passes, first_in_order


def key_mask(keys, bits):
    return keys.astype(np.uint64) & np.uint64((1 << bits) - 1)


def sort_reference(perm, passes):
    """the order KeySort documents: perm, then a stable sort by each pass's masked keys, least significant first"""
    order = np.asarray(perm, dtype=np.uint32)
    for keys, bits in passes:
        order = order[np.argsort(key_mask(keys, bits)[order], kind="stable")]
    return order
