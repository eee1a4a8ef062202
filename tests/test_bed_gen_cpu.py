"""The inputs of tests/test_gpu_bed_device.py checked without a GPU: on every dense row set the host twin of the BED
merges (bed.cpp) answers as the oracle does, both wrap `curr_end + merge_distance` as the reference's release build
does, and the plain statements of bed_gen.py (text of a row, piece count) say what they should on hand-made cases."""
import numpy as np

import impg_amd
from impg_amd import index as gi
from oracle import oracle as o
from tests import bed_gen


def test_dense_sets_are_dense_and_stable():
    sets = bed_gen.dense_sets()
    assert len(sets) == len(bed_gen.DENSE_GRID) * bed_gen.SETS_PER_CELL == 6048
    assert sum(len(s) for s in sets) <= 78624 and max(len(s) for s in sets) == bed_gen.MAX_ROWS
    assert any(len(s) == 0 for s in sets) and any(len(s) == 1 for s in sets)
    again = bed_gen.dense_sets()
    assert all(a.tolist() == b.tolist() for a, b in zip(sets, again))
    allrows = np.concatenate(sets)
    assert (allrows["q_first"] == allrows["q_last"]).any() and (np.minimum(allrows["q_first"], allrows["q_last"]) < 0).any()
    assert (allrows["q_first"] > allrows["q_last"]).any() and (allrows["t_first"] < allrows["t_last"]).all()
    # the tie rules need collisions: most sets of several rows hold two rows with one start
    several = [s for s in sets if len(s) >= 6]
    shared = sum(len(set(np.minimum(s["q_first"], s["q_last"]).tolist())) < len(s) for s in several)
    assert shared > len(several) // 2


def test_host_twin_matches_oracle_on_every_dense_set():
    for k, iv in enumerate(bed_gen.dense_sets()):
        ov = iv.astype(o.INTERVAL_DTYPE)
        for d, ms in bed_gen.MODES:
            got = gi.bed_merge(iv, d, ms)
            want = o.bed_merge(ov, d, ms)
            assert got.tolist() == want.tolist(), (k, d, ms, iv.tolist())


def test_gap_2d_export_is_the_first_stage():
    """oracle.merge_gap_2d followed by oracle.merge_query is oracle.bed_merge"""
    for iv in bed_gen.dense_sets()[::7]:
        ov = iv.astype(o.INTERVAL_DTYPE)
        for d in bed_gen.DISTANCES:
            first = o.merge_gap_2d(ov, d)
            assert len(first) <= len(ov)
            assert o.merge_query(first, d, True).tolist() == o.bed_merge(ov, d, True).tolist()


def test_overflow_pair_wraps_like_the_reference():
    iv = bed_gen.intervals(bed_gen.OVERFLOW_PAIR)
    for d, n_out in bed_gen.OVERFLOW_CASES:
        for ms in (True, False):
            host = gi.bed_merge(iv, d, ms)
            want = o.bed_merge(iv.astype(o.INTERVAL_DTYPE), d, ms)
            assert len(host) == n_out and len(want) == n_out, (d, ms, host.tolist(), want.tolist())
            assert host.tolist() == want.tolist()
    one = gi.bed_merge(iv, 147483547, True)
    assert (int(one["q_first"][0]), int(one["q_last"][0])) == (2000000000, 2000000600)


def test_expected_line():
    names = ["a", "chr1:999-5000", "x:+7-9", "y:-7-9", "z:12", "w:2147483648-1", "s#1#c:5-"]
    line = bed_gen.expected_line
    assert line(0, 1, 2, 0, "r", names, True) == b"a\t1\t2\tr\t.\t+\n"
    assert line(1, 1, 9001, 1, "", names, True) == b"chr1\t1000\t10000\t\t.\t-\n"
    assert line(1, 1, 9001, 1, "", names, False) == b"chr1:999-5000\t1\t9001\t\t.\t-\n"
    assert line(2, 0, 1, 0, "r", names, True) == b"x\t7\t8\tr\t.\t+\n"
    for k in (3, 4, 5):  # a sign that is a dash, no dash, a number beyond i32: the name stays whole
        assert line(k, 0, 1, 0, "r", names, True) == names[k].encode() + b"\t0\t1\tr\t.\t+\n"
    assert line(6, 0, 1, 0, "r", names, True) == b"s#1#c\t5\t6\tr\t.\t+\n"
    assert line(1, -1, -2 ** 31, 0, "r", names, True) == b"chr1\t998\t2147484647\tr\t.\t+\n"  # the shift wraps 2^32
    assert line(7, -1, -2 ** 31, 0, "r", names, True) == b"7\t4294967295\t2147483648\tr\t.\t+\n"
    assert line(4294967295, 0, 0, 0, "r", names, True) == b"4294967295\t0\t0\tr\t.\t+\n"
    for name in ["a:1-2", "a:b:10-20", "a:+7-9", "a:-7-9", "a:7", ":5-6", "a:2147483647-1", "a:2147483648-1", "a:00012-3", "a:1-2:x", "", ":"]:
        want = o.parse_subsequence(name)
        got = bed_gen.subsequence_origin(name)
        assert (got is None and want is None) or (want is not None and got == (want[0], want[1])), (name, got, want)


def test_piece_count():
    pc = bed_gen.piece_count
    assert pc([], 64) == 0
    assert pc([10, 10, 10], 64) == 1 and pc([10, 10, 10], 30) == 1 and pc([10, 10, 10], 29) == 2 and pc([10, 10, 10], 10) == 3
    assert pc([10, 10, 10], 9) == 3 and pc([100], 64) == 1  # at least one row a piece
    assert pc([60, 5, 60, 5], 64) == 4 and pc([60, 4, 60, 4], 64) == 2 and pc([60, 4, 1, 60], 64) == 2 and pc([60, 4, 1, 60], 63) == 3
    assert pc([64, 64], 64) == 2 and pc([64, 1], 64) == 2 and pc([63, 1], 64) == 1
