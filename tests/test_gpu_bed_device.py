"""The device BED merges and text (impg_amd/csrc/bed_device.hip) on their own, through impg_gpu_selftest_bed_rows: the rows
of tests/bed_gen.py instead of a query's.  Merged rows, the rows between the two merges and the bed_* counters against
the oracle (oracle.bed_merge, oracle.merge_gap_2d); the text against bed_gen.expected_line; the text stream's pieces
against bed_gen.piece_count.  Every case is small."""
import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import bed_gen
from tests.paf_gen import random_paf, random_ranges
from tests.test_gpu_parity import _bed_three_ways, both

pytestmark = pytest.mark.gpu

LONG_NAME = "L" * 300
SEQ_NAMES = ["s", LONG_NAME, "base:999-5000", "wrap:2147483647-9", "chrC:oops-5"]
DEFAULT_PIECE = 256 << 20


@pytest.fixture(scope="module")
def g(tmp_path_factory):
    """a handle whose sequence names are the text tests': 1 and 300 bytes, two "base:START-END" names, one that is none"""
    lines = ["%s\t6000\t0\t100\t+\t%s\t6000\t0\t100\t100\t100\t60\tcg:Z:100=" % (SEQ_NAMES[k], SEQ_NAMES[(k + 1) % len(SEQ_NAMES)])
             for k in range(len(SEQ_NAMES))]
    path = str(tmp_path_factory.mktemp("bed_device") / "names.paf")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    h = impg_amd.GpuImpg.from_paf(path)
    assert sorted(h.seq_name(i) for i in range(h.num_seqs())) == sorted(SEQ_NAMES)
    return h


@pytest.fixture(scope="module")
def nameless():
    """a handle without sequence names: every id prints as a decimal"""
    rec, ops, sl = impg_amd.synth_paf(1, 10, n_seq=4, seq_len=100000, target_span=2000, n_blocks=10)
    h = impg_amd.GpuImpg.from_records(rec, ops, sl)
    assert h.seq_name(0) is None
    return h


def names_of(h):
    return [h.seq_name(i) for i in range(h.num_seqs()) if h.seq_name(i) is not None]


@pytest.fixture(scope="module")
def dense():
    """the dense sets and, once for all tests, what the oracle makes of each under every (d, merge_strands)"""
    sets = bed_gen.dense_sets()
    osets = [s.astype(o.INTERVAL_DTYPE) for s in sets]
    want = {(d, ms): [[bed_gen.merged_tuple(x) for x in o.bed_merge(s, d, ms)] for s in osets] for d, ms in bed_gen.MODES}
    gap = {d: [o.merge_gap_2d(s, d).tolist() for s in osets] for d in bed_gen.DISTANCES}
    return sets, want, gap


def by_range(merged, n_ranges):
    """merged rows -> per range [(query id, start, end, strand)], in output order; the rows come grouped by range"""
    r = merged["range"].astype(np.int64)
    assert (np.diff(r) >= 0).all() and (len(r) == 0 or r[-1] < n_ranges)
    out = [[] for _ in range(n_ranges)]
    for k, x in zip(r.tolist(), merged.tolist()):
        out[k].append((x[1], x[2], x[3], x[4]))
    return out


def gap_by_range(rows, rng, n_ranges):
    """the rows between the merges -> per range, in their order (a range's rows need not be adjacent)"""
    out = [[] for _ in range(n_ranges)]
    for k, x in zip(rng.tolist(), rows.tolist()):
        out[k].append(tuple(x))
    return out


def text_of(merged, range_names, names, original=False):
    return b"".join(bed_gen.expected_line(x[1], x[2], x[3], x[4], range_names[x[0]], names, original) for x in merged.tolist())


def counters(h):
    return {k: h.counter(k) for k in ("bed_rows", "bed_gap_roots", "bed_runs", "bed_text_pieces", "bed_text_bytes")}


# ---- dense sets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ms", bed_gen.MODES)
def test_dense_sets(g, dense, d, ms):
    """~6 000 ranges of 0 .. 13 colliding rows in one call: every range's merged rows are the oracle's, in order; so are
    the rows between the two merges (oracle.merge_gap_2d: the chain stands where its first row stood); the counters are
    the oracle's sums; the text is the statement of bed_gen.expected_line."""
    sets, want, gap = dense
    rows, rr = bed_gen.batch(sets)
    merged, text, grows, grange = g.bed_rows(rows, rr, len(sets), 2, d, ms, gap=True)
    got = by_range(merged, len(sets))
    bad = [k for k in range(len(sets)) if got[k] != want[(d, ms)][k]]
    assert not bad, (d, ms, bad[0], sets[bad[0]].tolist(), got[bad[0]], want[(d, ms)][bad[0]])
    ggot = gap_by_range(grows, grange, len(sets))
    bad = [k for k in range(len(sets)) if ggot[k] != [tuple(x) for x in gap[d][k]]]
    assert not bad, (d, bad[0], sets[bad[0]].tolist(), ggot[bad[0]], gap[d][bad[0]])
    c = counters(g)
    assert c["bed_rows"] == len(rows) and c["bed_gap_roots"] == sum(len(x) for x in gap[d])
    assert c["bed_runs"] == sum(len(x) for x in want[(d, ms)]) == len(merged)
    assert text == text_of(merged, [str(k) for k in range(len(sets))], names_of(g))
    assert c["bed_text_bytes"] == len(text) and c["bed_text_pieces"] == 1


# ---- chunk shape ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ms", [(0, True), (2, False), (5, True), (-1, True)])
def test_range_order_and_interleaving_do_not_show(g, dense, d, ms):
    """the same sets as ranges in reversed order, and with the rows of different ranges interleaved in the input array:
    every set's merged rows are what they were"""
    sets, want, _ = dense
    n = len(sets)
    rev = list(range(n - 1, -1, -1))
    for order, interleave in ((rev, False), (None, True), (rev, True)):
        rows, rr = bed_gen.batch(sets, order, interleave)
        if interleave:
            assert (np.diff(rr.astype(np.int64)) < 0).any()
        merged, _ = g.bed_rows(rows, rr, n, 2, d, ms)
        got = by_range(merged, n)
        for k in range(n):
            assert got[order[k] if order else k] == want[(d, ms)][k], (order is not None, interleave, k, sets[k].tolist())


# ---- contention ---------------------------------------------------------------------------------------------------
def contention_sets():
    rng = np.random.default_rng(77)
    n = 2000
    out = []
    for rev in (False, True):
        # one group, every pair within d = 5000 on both axes: no early break, every thread walks the whole group
        a = np.zeros(n, dtype=impg_amd.INTERVAL_DTYPE)
        s = rng.integers(0, 1000, n)
        ln = rng.integers(500, 1500, n)
        a["q_first"], a["q_last"] = (s + ln, s) if rev else (s, s + ln)
        t = rng.integers(0, 1000, n)
        a["t_first"], a["t_last"] = t, t + rng.integers(500, 1500, n)
        out.append(a)
        # 1 000 chains of two rows, 100 000 apart from each other.  A chain's rows are emitted up to 2 000 slots apart
        # (the second block is permuted) and either of the two comes first, so every union races with its neighbours' and
        # the chain's slot is not always the row the sort meets first.  On '-' the reference links contained rows only.
        b = np.zeros(n, dtype=impg_amd.INTERVAL_DTYPE)
        chain = np.concatenate([np.arange(n // 2), rng.permutation(n // 2)])
        member = np.concatenate([np.arange(n // 2) % 2, 1 - chain[n // 2:] % 2])  # 0: the row the other one follows
        c = chain * 100000
        if rev:
            b["q_first"], b["q_last"] = np.where(member == 0, c + 300, c + 200), np.where(member == 0, c, c + 100)
            b["t_first"] = np.where(member == 0, c + 150, c)
        else:
            b["q_first"], b["q_last"] = np.where(member == 0, c, c + 150), np.where(member == 0, c + 100, c + 250)
            b["t_first"] = np.where(member == 0, c, c + 150)
        b["t_last"] = b["t_first"] + 100
        b["query_id"] = chain % 2
        out.append(b)
    return out


@pytest.mark.parametrize("ms", [True, False])
def test_contention(g, ms):
    """a group of 2 000 rows that all link, and 1 000 two-row chains interleaved, on both strands: merged rows as the
    oracle has them, and every chain in the slot of its first row (the rows between the merges, in order)"""
    sets = contention_sets()
    rows, rr = bed_gen.batch(sets)
    for d in (5000, 60):
        merged, _, grows, grange = g.bed_rows(rows, rr, len(sets), 2, d, ms, gap=True)
        got, ggot = by_range(merged, len(sets)), gap_by_range(grows, grange, len(sets))
        for k, s in enumerate(sets):
            so = s.astype(o.INTERVAL_DTYPE)
            wgap = [tuple(x) for x in o.merge_gap_2d(so, d).tolist()]
            assert ggot[k] == wgap, (d, k)
            assert got[k] == [bed_gen.merged_tuple(x) for x in o.bed_merge(so, d, ms)], (d, k)
            if d == 60 and k % 2 == 1:
                assert len(wgap) == 1000  # (the case is what it says: every chain links, none links another)
            if d == 5000 and k % 2 == 0:
                assert len(wgap) < 20


# ---- no-merge branch --------------------------------------------------------------------------------------------------
def test_no_merge_branch(g, dense):
    sets, want, _ = dense
    sets = sets[::5]
    n = len(sets)
    for interleave in (False, True):
        rows, rr = bed_gen.batch(sets, None, interleave)
        # d = -1 and the strands kept apart: rows unchanged, grouped by range, in emission order
        merged, text = g.bed_rows(rows, rr, n, 2, -1, False)
        got = by_range(merged, n)
        for k, s in enumerate(sets):
            assert got[k] == [bed_gen.merged_tuple(x) for x in s], (k, interleave)
        assert counters(g)["bed_runs"] == len(rows) == counters(g)["bed_gap_roots"]
        # d = -1 and the strands merged: the sweep runs and keeps every row apart -- each its own run, ending at its own end
        merged, text = g.bed_rows(rows, rr, n, 2, -1, True)
        got = by_range(merged, n)
        for k, s in enumerate(sets):
            assert sorted(got[k]) == sorted(bed_gen.merged_tuple(x) for x in s), (k, interleave)
            assert got[k] == [bed_gen.merged_tuple(x) for x in o.bed_merge(s.astype(o.INTERVAL_DTYPE), -1, True)], (k, interleave)


# ---- where the sorts' guards stand ------------------------------------------------------------------------------------
def tied_rows(n=257):
    """n forward rows of one range that are equal on every sort key of both merges (sequences, strand, q_first = start)
    and differ in their ends and targets: only emission order tells them apart.  One more than a block of threads."""
    rng = np.random.default_rng(257)
    a = np.zeros(n, dtype=impg_amd.INTERVAL_DTYPE)
    a["q_first"], a["q_last"] = 100, 100 + rng.integers(0, 50, n)
    t = rng.integers(0, 300, n)
    a["t_first"], a["t_last"] = t, t + rng.integers(1, 20, n)
    assert (np.diff(a["q_last"]) < 0).any() and (np.diff(a["t_first"]) < 0).any()  # (no key would have put them in this order)
    return a


GUARD_SETS = {"one row": [bed_gen.intervals([(1, 30, 20, 0, 5, 9)])],
              "two rows in two ranges": [bed_gen.intervals([(0, 10, 20, 1, 5, 9)]), bed_gen.intervals([(0, 12, 18, 1, 7, 9)])],
              "257 tied rows": [tied_rows()]}


@pytest.mark.parametrize("d", [-1, 0, 5])
@pytest.mark.parametrize("ms", [True, False])
@pytest.mark.parametrize("case", sorted(GUARD_SETS))
def test_sort_guard_edges(g, case, d, ms):
    """a call of one row (no gap_2d sort), one of two rows that share no range, and 257 rows that tie on every key of
    every pass: merged rows, the rows between the merges, counters and text as the oracle and bed_gen state them"""
    sets = GUARD_SETS[case]
    rows, rr = bed_gen.batch(sets)
    merged, text, grows, grange = g.bed_rows(rows, rr, len(sets), 2, d, ms, gap=True)
    got, ggot = by_range(merged, len(sets)), gap_by_range(grows, grange, len(sets))
    for k, s in enumerate(sets):
        so = s.astype(o.INTERVAL_DTYPE)
        assert ggot[k] == [tuple(x) for x in o.merge_gap_2d(so, d).tolist()], (case, d, k)
        assert got[k] == [bed_gen.merged_tuple(x) for x in o.bed_merge(so, d, ms)], (case, d, ms, k)
    if d < 0 and not ms:
        assert [x for r in got for x in r] == [bed_gen.merged_tuple(x) for x in rows]  # untouched, in emission order
    c = counters(g)
    assert c["bed_rows"] == len(rows) and c["bed_gap_roots"] == len(grows) and c["bed_runs"] == len(merged)
    assert text == text_of(merged, [str(k) for k in range(len(sets))], names_of(g)) and c["bed_text_bytes"] == len(text)


# ---- overflow -----------------------------------------------------------------------------------------------------
def test_overflow_pair_on_the_device(g):
    iv = bed_gen.intervals(bed_gen.OVERFLOW_PAIR)
    for d, n_out in bed_gen.OVERFLOW_CASES:
        for ms in (True, False):
            merged, _ = g.bed_rows(iv, np.zeros(2, dtype=np.uint32), 1, 2, d, ms)
            want = [bed_gen.merged_tuple(x) for x in o.bed_merge(iv.astype(o.INTERVAL_DTYPE), d, ms)]
            assert len(want) == n_out and by_range(merged, 1)[0] == want, (d, ms, merged.tolist())


def test_overflow_pair_through_a_query(tmp_path):
    """two alignments near 2 Gbp on a sequence of 2 100 000 000: query_batch_bed (device) == results.bed() (host) == oracle"""
    L = 2100000000
    lines = ["Q\t%d\t%d\t%d\t+\tT\t%d\t%d\t%d\t100\t100\t60\tcg:Z:100=" % (L, qs, qs + 100, L, ts, ts + 100)
             for qs, ts in ((2000000000, 3000), (2000000500, 1000))]  # (the target runs backwards: gap_2d leaves them apart)
    try:
        gq, c = both(tmp_path, "\n".join(lines) + "\n", bidirectional=False)
    except impg_amd.ImpgGpuError as e:
        pytest.skip("an index over a sequence of 2 100 000 000 cannot be built: %s" % e)
    T = gq.seq_id("T")
    for d, n_out in bed_gen.OVERFLOW_CASES:
        for kw in (dict(), dict(consider_strandness=True)):
            text = _bed_three_ways(gq, c, [(T, 0, 5000)], ["r"], d, **kw)
            assert len([ln for ln in text.splitlines() if ln.startswith("Q\t")]) == n_out, (d, text)


# ---- key width ----------------------------------------------------------------------------------------------------
def test_key_width_64_bits_and_one_more(g):
    top = 2 ** 31
    ids = [0, 1, top - 2, top - 1]
    rng = np.random.default_rng(5)
    sets = []
    for _ in range(3):
        n = 40
        a = np.zeros(n, dtype=impg_amd.INTERVAL_DTYPE)
        a["query_id"] = rng.choice(ids, n)
        a["target_id"] = rng.choice(ids, n)
        s = rng.integers(0, 30, n)
        ln = rng.integers(0, 4, n)
        rev = rng.random(n) < 0.4
        a["q_first"], a["q_last"] = np.where(rev, s + ln, s), np.where(rev, s, s + ln)
        t = rng.integers(0, 30, n)
        a["t_first"], a["t_last"] = t, t + rng.integers(1, 4, n)
        sets.append(a)
    for d, ms in ((0, True), (2, True), (2, False)):
        # 2 ranges: 1 + 31 + 31 + 1 = 64 bits
        rows, rr = bed_gen.batch(sets[:2], None, True)
        merged, text, grows, grange = g.bed_rows(rows, rr, 2, top, d, ms, gap=True)
        got, ggot = by_range(merged, 2), gap_by_range(grows, grange, 2)
        for k in range(2):
            so = sets[k].astype(o.INTERVAL_DTYPE)
            assert got[k] == [bed_gen.merged_tuple(x) for x in o.bed_merge(so, d, ms)], (d, ms, k)
            assert ggot[k] == [tuple(x) for x in o.merge_gap_2d(so, d).tolist()], (d, k)
        assert {x[1] for x in merged.tolist()} == set(ids)
        assert text == text_of(merged, ["0", "1"], names_of(g))
        # 3 ranges: 65 bits
        rows, rr = bed_gen.batch(sets)
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            g.bed_rows(rows, rr, 3, top, d, ms)
        assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED and "too many sequences for the device-side BED merge" in str(ei.value)
    # the handle answers the next call
    merged, _ = g.bed_rows(sets[0], np.zeros(len(sets[0]), dtype=np.uint32), 1, top, 2, True)
    assert by_range(merged, 1)[0] == [bed_gen.merged_tuple(x) for x in o.bed_merge(sets[0].astype(o.INTERVAL_DTYPE), 2, True)]


def test_refusals(g):
    iv = bed_gen.intervals([(0, 1, 2, 1, 3, 4), (1, 5, 6, 0, 7, 8)])
    for rr, n_ranges, n_seq in (([0, 1], 1, 2), ([0, 0], 1, 1), ([0, 2], 2, 2)):
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            g.bed_rows(iv, np.array(rr, dtype=np.uint32), n_ranges, n_seq, 0, True)
        assert ei.value.code == impg_amd.IMPG_E_INVALID
    bad = iv.copy()
    bad["target_id"][1] = 2
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        g.bed_rows(bad, np.zeros(2, dtype=np.uint32), 1, 2, 0, True)
    assert ei.value.code == impg_amd.IMPG_E_INVALID
    merged, text = g.bed_rows(iv[:0], np.zeros(0, dtype=np.uint32), 3, 2, 0, True)
    assert len(merged) == 0 and text == b"" and counters(g) == dict.fromkeys(counters(g), 0)


def test_refuses_a_multi_handle(tmp_path):
    text, _ = random_paf(77, 60, n_seq=5, seq_len=20000, self_aln=True)
    path = str(tmp_path / "w.paf")
    with open(path, "w") as f:
        f.write(text)
    m = impg_amd.GpuImpg.from_paf(path, devices=[0, 0], lanes=1)
    iv = bed_gen.intervals([(0, 1, 2, 1, 3, 4)])
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        m.bed_rows(iv, np.zeros(1, dtype=np.uint32), 1, 2, 0, True)
    assert ei.value.code == impg_amd.IMPG_E_INVALID


# ---- text widths ----------------------------------------------------------------------------------------------------
WIDTH_VALUES = sorted({-2 ** 31, -1, 0, 2 ** 31 - 1} | {10 ** k - 1 for k in range(1, 10)} | {10 ** k for k in range(1, 10)})


def width_rows(ids):
    """every value of WIDTH_VALUES as a start and as an end, on both strands, for every id; unchanged by the no-merge
    branch, so the printed rows are these"""
    rows = []
    for q in ids:
        for a, b in list(zip(WIDTH_VALUES, WIDTH_VALUES[1:])) + [(v, v) for v in WIDTH_VALUES] + [(WIDTH_VALUES[0], WIDTH_VALUES[-1])]:
            rows.append((q, a, b, 0, 0, 1))
            if a != b:
                rows.append((q, b, a, 0, 0, 1))
    return bed_gen.intervals(rows)


@pytest.mark.parametrize("original", [False, True])
def test_text_widths_named(g, original):
    """decimal widths at every power of ten, coordinates below zero printed as u32, names of 1 and 300 bytes, a shift
    that carries 999 / 9 999 ... across a power of ten and one that wraps 2^32, range names of 0 and 300 bytes"""
    names = names_of(g)
    iv = width_rows(range(len(names)))
    rr = (np.arange(len(iv)) % 3).astype(np.uint32)
    rnames = ["", "R" * 300, "mid"]
    merged, text = g.bed_rows(iv, rr, 3, len(names), -1, False, original_sequence_coordinates=original, range_names=rnames)
    assert [tuple(x)[1:] for x in merged.tolist()] == [bed_gen.merged_tuple(x) for k in range(3) for x in iv[rr == k]]
    want = text_of(merged, rnames, names, original)
    assert text == want
    if original:
        assert b"base\t999\t" in text and b"base\t10998\t" in text and b"base\t998\t" in text and b"wrap\t2147483646\t" in text and b"base:999" not in text
    else:
        assert b"base:999-5000\t4294967295\t" in text and b"\t2147483648\t" in text
    assert (LONG_NAME.encode() + b"\t") in text and b"\ns\t" in text and b"\t\t.\t+\n" in text and b"\t\t.\t-\n" in text


def test_text_widths_unnamed(nameless):
    """ids without names print as decimals: 0, 9, 10 and 4294967295 (an id universe of 2^32: the no-merge branch builds no
    key from it)"""
    iv = width_rows([0, 9, 10, 4294967295])
    rr = np.zeros(len(iv), dtype=np.uint32)
    for original in (False, True):
        merged, text = nameless.bed_rows(iv, rr, 1, 2 ** 32, -1, False, original_sequence_coordinates=original, range_names=["r"])
        assert [tuple(x)[1:] for x in merged.tolist()] == [bed_gen.merged_tuple(x) for x in iv]
        assert text == text_of(merged, ["r"], [], original)
        assert b"\n4294967295\t4294967295\t" in text and text.startswith(b"0\t2147483648\t4294967295\tr\t.\t+\n")


# ---- pieces ---------------------------------------------------------------------------------------------------------
def test_text_pieces(g):
    """the same ~3 000 printed rows at every piece size: identical bytes, the greedy number of pieces"""
    names = names_of(g)
    rng = np.random.default_rng(9)
    n = 3000
    iv = np.zeros(n, dtype=impg_amd.INTERVAL_DTYPE)
    iv["query_id"] = rng.integers(0, len(names) + 3, n)
    a = rng.integers(0, 10 ** rng.integers(1, 10, n))
    iv["q_first"], iv["q_last"] = a, a + rng.integers(0, 1000, n)
    iv["t_last"] = 1
    n_ranges = 50
    rr = np.sort(rng.integers(0, n_ranges, n)).astype(np.uint32)
    rnames = ["n" * int(k) for k in rng.integers(0, 40, n_ranges)]
    merged, want = g.bed_rows(iv, rr, n_ranges, len(names) + 3, -1, False, range_names=rnames)
    assert want == text_of(merged, rnames, names) and len(merged) == n
    lengths = [len(ln) + 1 for ln in want.split(b"\n")[:-1]]
    total = len(want)
    assert sum(lengths) == total and max(lengths) > 300 and total > 64 * 1024
    try:
        for piece in (64, 100, 4096, total - 1, total, total + 1, DEFAULT_PIECE):
            g.set_option("bed_text_piece_bytes", piece)
            merged, text = g.bed_rows(iv, rr, n_ranges, len(names) + 3, -1, False, range_names=rnames)
            assert text == want, piece
            c = counters(g)
            assert c["bed_text_pieces"] == bed_gen.piece_count(lengths, piece), piece
            assert c["bed_text_bytes"] == total, piece
        assert bed_gen.piece_count(lengths, 64) > n // 2 and bed_gen.piece_count(lengths, total - 1) == 2 and bed_gen.piece_count(lengths, total) == 1
        # one row longer than the text buffer of a 64-byte piece: refused before anything is queued, and the handle goes on
        one = bed_gen.intervals([(0, 5, 6, 0, 0, 1)])
        g.set_option("bed_text_piece_bytes", 64)
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            g.bed_rows(one, np.zeros(1, dtype=np.uint32), 1, 1, -1, False, range_names=["N" * 6000])
        assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED and "a single BED row longer than the text buffer" in str(ei.value)
        g.set_option("bed_text_piece_bytes", DEFAULT_PIECE)
        merged, text = g.bed_rows(one, np.zeros(1, dtype=np.uint32), 1, 1, -1, False, range_names=["N" * 6000])
        assert text == bed_gen.expected_line(0, 5, 6, 0, "N" * 6000, names, False)
    finally:
        g.set_option("bed_text_piece_bytes", DEFAULT_PIECE)


# ---- through queries ------------------------------------------------------------------------------------------------
def test_query_with_inconsistent_cigars(tmp_path):
    """records whose coordinates disagree with their CIGAR (and zero-length ops) through the device path, whole and in
    chunks of 7 ranges whose text takes several pieces"""
    text, _ = random_paf(21, 500, n_seq=5, seq_len=30000, self_aln=True, inconsistent=True, weird=True)
    gq, c = both(tmp_path, text)
    ranges = random_ranges(21, 40, 5, 30000, max_len=5000, min_len=150)
    names = [None if i % 3 else "n%d" % i for i in range(len(ranges))]
    modes = (dict(), dict(transitive=True, max_depth=3, min_transitive_len=20), dict(transitive=True, max_depth=2, consider_strandness=True))
    whole = {}
    for d in (-1, 0, 25, 1000):
        for k, kw in enumerate(modes):
            whole[(d, k)] = _bed_three_ways(gq, c, ranges, names, d, **kw)
    gq.set_option("chunk_ranges", 7)
    gq.set_option("bed_text_piece_bytes", 4096)
    for d in (-1, 25):
        for k, kw in enumerate(modes):
            assert _bed_three_ways(gq, c, ranges, names, d, **kw) == whole[(d, k)]
    assert gq.counter("bed_text_pieces") > 1


def test_query_original_sequence_coordinates(tmp_path):
    """the renamed index of test_original_sequence_coordinates through the device text, 30 ranges, whole and in chunks"""
    text, _ = random_paf(141, 200, n_seq=6, seq_len=20000, self_aln=True)
    ren = {"s0": "chrA:1000-21000", "s1": "sample#1#chrB:5-20005", "s2": "chrC:oops-5"}
    lines = []
    for ln in text.splitlines():
        f = ln.split("\t")
        f[0], f[5] = ren.get(f[0], f[0]), ren.get(f[5], f[5])
        lines.append("\t".join(f))
    gq, c = both(tmp_path, "\n".join(lines) + "\n")
    ranges = random_ranges(9, 30, 6, 20000, max_len=3000, min_len=150)
    rnames = ["r%d" % i for i in range(len(ranges))]
    kw = dict(transitive=True, max_depth=2, min_transitive_len=40, original_sequence_coordinates=True)
    whole = _bed_three_ways(gq, c, ranges, rnames, 20, **kw)
    assert "chrA\t" in whole and "chrA:1000-21000\t" not in whole and "sample#1#chrB\t" in whole and "chrC:oops-5\t" in whole
    gq.set_option("chunk_ranges", 7)
    gq.set_option("bed_text_piece_bytes", 4096)
    assert _bed_three_ways(gq, c, ranges, rnames, 20, **kw) == whole
    assert gq.counter("bed_text_pieces") > 1
