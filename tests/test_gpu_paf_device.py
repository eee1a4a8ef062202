"""impg_gpu_query_batch_paf (impg_amd/csrc/paf_device.inc): query, merge_adjusted_intervals, the merged CIGARs fused and the
PAF text on the device.  Every comparison is three-way where the oracle can take part: device text == host route
(query_batch with store_cigar + .paf(fmt="paf")) == oracle; the counters against the model of tests/paf_ref.py, which
tests/test_paf_ref_cpu.py holds against the oracle.  Every case is small."""
import os
import subprocess
import threading

import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import bedpe_ref, paf_ref as ref
from tests.paf_gen import random_paf, random_ranges
from tests.tp_gen import random_tp

pytestmark = pytest.mark.gpu

GROUP = 4  # lanes per element of the cg passes: 2 ** (option "paf_group_log2", by default)
COUNTER_KEYS = ref.COUNTERS + ("paf_text_pieces",)


def counters(g):
    return {k: g.counter(k) for k in COUNTER_KEYS}


def write(tmp, name, text):
    path = str(tmp / name)
    with open(path, "w") as f:
        f.write(text)
    return path


def both(tmp, name, text, **kw):
    path = write(tmp, name, text)
    return impg_amd.GpuImpg.from_paf(path, **kw), o.OracleIndex(paf_paths=[path], preparse=True, **kw)


def host_text(g, ranges, rnames, d, subset_keep=None, **kw):
    p = impg_amd.make_params(store_cigar=True, **kw)
    return g.query_batch(ranges, p, subset_keep=subset_keep).paf(rnames, merge_distance=d, params=p, fmt="paf")


def oracle_text(c, ranges, rnames, d, **kw):
    return "".join(c.query_paf(c.seq_name(t), s, e, range_name=rn, merge_distance=d, fmt="paf", **kw) for (t, s, e), rn in zip(ranges, rnames))


def three_way(g, c, ranges, rnames, d, **kw):
    got = g.query_batch_paf(ranges, impg_amd.make_params(**kw), merge_distance=d, range_names=rnames)
    assert got == oracle_text(c, ranges, rnames, d, **kw), (d, kw)
    assert got == host_text(g, ranges, rnames, d, **kw), (d, kw)
    return got


def model_counters(c, ranges, rnames, d, **kw):
    tally = ref.new_counters()
    for (t, s, e), rn in zip(ranges, rnames):
        rows, cigars = c.query_cigar(t, s, e, **kw)
        rows = [(r["query_id"], r["q_first"], r["q_last"], r["target_id"], r["t_first"], r["t_last"]) for r in rows]
        ref.paf_range(rows, cigars, d, rn, c.seq_name, c.seq_len, transitive=bool(kw.get("transitive")), counters=tally)
    return tally


def same_counters(g, tally):
    have = counters(g)
    assert {k: have[k] for k in ref.COUNTERS} == {k: tally[k] for k in ref.COUNTERS}
    return have


def cg_fields(text):
    return [ln.split("\tcg:Z:")[1].split("\t")[0] for ln in text.splitlines()]


# ---- dense sets -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    """20 dense tilings side by side in one index (their sequences told apart by a prefix) and all their ranges"""
    texts, ranges = [], []
    for seed in range(20):
        text, rs = bedpe_ref.dense_paf(seed, prefix="k%d_" % seed)
        texts.append(text)
        ranges.append((seed, rs))
    g, c = both(tmp_path_factory.mktemp("paf_dense"), "dense.paf", "".join(texts))
    rl = [(g.seq_id("k%d_%s" % (seed, bedpe_ref.DENSE_NAMES[t])), s, e) for seed, rs in ranges for (t, s, e) in rs]
    assert all(g.seq_name(t) == c.seq_name(t) for t, _, _ in rl)
    return g, c, rl, ["r%d" % i for i in range(len(rl))]


@pytest.mark.parametrize("d", [-1, 0, 1, 2, 5, 100])
def test_dense_sets(dense, d):
    """60 ranges over tilings whose blocks lie 0, 1, 2, 5 or -1 bases apart, in one call: the text three ways, and the
    counters are the model's sums -- both join kinds, both strands, fusing across joins and inside rows."""
    g, c, rl, rnames = dense
    got = three_way(g, c, rl, rnames, d)
    want = model_counters(c, rl, rnames, d)
    have = same_counters(g, want)
    assert have["paf_text_bytes"] == len(got) and have["paf_text_pieces"] == 1
    if d >= 5:
        assert want["paf_joins_contiguous"] >= 50 and want["paf_joins_gap"] >= 50 and want["reverse_multi_runs"] >= 50
        assert want["paf_ops_printed"] < want["paf_ops_read"] + 2 * want["paf_joins_gap"]  # (a gap join adds an op or two: some ops were fused)
    if d < 0:
        assert have["paf_runs"] == have["paf_rows"] and have["paf_ops_printed"] == have["paf_ops_read"] and have["paf_through_rows"] == 0


# ---- cg kernel edges ----------------------------------------------------------------------------------------------------
def ops_of(rng, n_ops):
    """n_ops random ops as (length, code letter), neighbours of one code allowed (they fuse once the row is joined)"""
    return [(int(rng.integers(1, 9)), "=XID"[int(rng.integers(0, 4))]) for _ in range(n_ops)]


def text_of(ops):
    return "".join("%d%s" % x for x in ops)


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    """CIGARs of 1, 2, G-1, G, G+1, 2G+1, 15-17, 33, 63-65, 129 and 1000 ops, each as two contiguous records that join at
    d = 0, the boundary pair of equal codes for every other size and of different codes for the rest; then, for every
    group width, a same-code group lying on ops G-1 .. G+1 of a record that a second one joins."""
    rng = np.random.default_rng(11)
    lines, ranges = [], []
    tpos, qpos = 1000, 500

    def record(ops):
        nonlocal tpos, qpos
        cg = text_of(ops)
        td, qd = bedpe_ref.cigar_spans(cg)
        lines.append("Q\t900000\t%d\t%d\t+\tT\t900000\t%d\t%d\t1\t1\t60\tcg:Z:%s" % (qpos, qpos + qd, tpos, tpos + td, cg))
        tpos, qpos = tpos + td, qpos + qd

    def pair(a, b):
        nonlocal tpos, qpos
        start = tpos
        record(a)
        record(b)
        ranges.append((start, tpos))
        tpos, qpos = tpos + 500, qpos + 700

    for i, n_ops in enumerate((1, 2, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1, 15, 16, 17, 33, 63, 64, 65, 129, 1000)):
        a, b = ops_of(rng, n_ops), ops_of(rng, n_ops)
        a[-1] = (a[-1][0], "=")  # (an '=' at the boundary also keeps both spans positive)
        b[0] = (b[0][0], "=" if i % 2 == 0 else "X")
        pair(a, b)
    for width in (4, 8, 16, 32, 64):
        a = [(1 + k % 3, "=X"[k % 2]) for k in range(width - 1)] + [(2, "I"), (3, "I"), (4, "I"), (5, "=")]
        pair(a, [(6, "="), (1, "X")])
    g, c = both(tmp_path_factory.mktemp("paf_edges"), "edges.paf", "\n".join(lines) + "\n", bidirectional=False)
    t = g.seq_id("T")
    rl = [(t, s, x) for s, x in ranges]
    return g, c, rl, ["e%d" % i for i in range(len(rl))]


def test_cg_kernel_edges(edges):
    g, c, rl, rnames = edges
    for d in (-1, 0, 5):
        got = three_way(g, c, rl, rnames, d, min_transitive_len=1)
        same_counters(g, model_counters(c, rl, rnames, d, min_transitive_len=1))
    assert g.counter("paf_joins_contiguous") == len(rl) == g.counter("paf_runs") and g.counter("paf_ops_read") > 2400
    assert g.counter("paf_ops_printed") < g.counter("paf_ops_read")
    assert all("2I3I4I" not in cg and "9I11=" in cg for cg in cg_fields(got)[-5:])  # the straddling group, and 5= + 6= behind it
    raw = g.query_batch_paf(rl, impg_amd.make_params(min_transitive_len=1), merge_distance=-1, range_names=rnames)
    assert sum("2I3I4I5=" in cg for cg in cg_fields(raw)) == 5  # (alone, the rows print raw)


def test_every_group_width_prints_the_same_text(edges):
    g, c, rl, rnames = edges
    p = impg_amd.make_params(min_transitive_len=1)
    try:
        for d in (-1, 5):
            want = g.query_batch_paf(rl, p, merge_distance=d, range_names=rnames)
            tally = counters(g)
            for lg in (3, 4, 5, 6, 2):  # 8 .. 64 lanes an element, and back to the default
                g.set_option("paf_group_log2", lg)
                assert g.query_batch_paf(rl, p, merge_distance=d, range_names=rnames) == want, (d, lg)
                assert counters(g) == tally, (d, lg)
        for bad in (1, 7):
            with pytest.raises(impg_amd.ImpgGpuError):
                g.set_option("paf_group_log2", bad)
    finally:
        g.set_option("paf_group_log2", 2)


def test_line_longer_than_the_piece(edges):
    """the 1000-op pair under a long range name prints a line of more than 64 + 4096 bytes: refused, with none of its chunk's
    text; with a chunk per range the call is refused all the same, and the next call answers"""
    g, c, rl, rnames = edges
    rnames = rnames[:14] + ["N" * 1500] + rnames[15:]
    p = impg_amd.make_params(min_transitive_len=1)
    want = g.query_batch_paf(rl, p, merge_distance=0, range_names=rnames)
    assert max(len(ln) for ln in want.splitlines()) > 64 + 4096
    try:
        g.set_option("bed_text_piece_bytes", 64)
        for chunk in (0, 1):
            g.set_option("chunk_ranges", chunk)
            with pytest.raises(impg_amd.ImpgGpuError) as ei:
                g.query_batch_paf(rl, p, merge_distance=0, range_names=rnames)
            assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED and "longer than the text buffer" in str(ei.value)
        short = [i for i in range(len(rl)) if i != 14]
        got = g.query_batch_paf([rl[i] for i in short], p, merge_distance=0, range_names=[rnames[i] for i in short])
        assert got == "".join(ln + "\n" for i, ln in enumerate(want.splitlines()) if i != 14)
        assert g.counter("paf_text_pieces") > 1
    finally:
        g.set_option("chunk_ranges", 0)
        g.set_option("bed_text_piece_bytes", 256 << 20)
    assert g.query_batch_paf(rl, p, merge_distance=0, range_names=rnames) == want


# ---- rows of our own (impg_gpu_selftest_paf_rows) -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    rec, ops, sl = impg_amd.synth_paf(1, 500, n_seq=4, seq_len=100000, target_span=2000, n_blocks=10)
    sl = sl.copy()
    sl[:] = (1 << 29) - 1
    return impg_amd.GpuImpg.from_records(rec, ops, sl)


SELF_ROW = (0, 100, 200, 0, 100, 200)


def run_rows(g, rows, cigars, d, **kw):
    """one range: the dropped row, then rows / cigars ('5=2I' strings); returns (device text, model text, model tally)"""
    allrows = [SELF_ROW] + list(rows)
    packed = [ref.pack("100=")] + [ref.pack(cg) for cg in cigars]
    got = g.selftest_paf_rows(np.array(allrows, dtype=impg_amd.INTERVAL_DTYPE), [0] * len(allrows), 1, packed, merge_distance=d,
                              range_names=["x"], **kw).decode()
    tally = ref.new_counters()
    name = lambda i: g.seq_name(i) if g.seq_name(i) is not None else str(i)
    want = ref.paf_range(allrows, packed, d, "x", name, g.seq_len, original=bool(kw.get("original_sequence_coordinates")), transitive=True,
                         counters=tally)
    assert got == want, (cigars, d)
    same_counters(g, tally)
    return got, tally


def tile(cigars, reverse=False, gaps=None, q0=1000, t0=5000):
    """rows that tile query sequence 1 and target sequence 0 with the given CIGARs, gaps[i] = (qd, td) in front of row i + 1"""
    rows = []
    q, t = q0, t0
    for i, cg in enumerate(cigars):
        td, qd = bedpe_ref.cigar_spans(cg)
        rows.append((1, q, q - qd, 0, t, t + td) if reverse else (1, q, q + qd, 0, t, t + td))
        gq, gt = gaps[i] if gaps and i < len(gaps) else (0, 0)
        q = q - qd - gq if reverse else q + qd + gq
        t = t + td + gt
    return rows


def test_intra_row_groups_and_gap_joins(plain):
    """groups inside a row print raw when the row is alone and fused when it is joined; a gap's I between a trailing and a
    leading I and its D likewise; a gap join on the reverse strand"""
    g = plain
    for cg, fused in (("5=2I3I10=", "5=5I10="), ("0=5=", "5="), ("4D4D12=", "8D12=")):
        got, _ = run_rows(g, tile([cg]), [cg], 0)
        assert cg_fields(got) == [cg]
        got, _ = run_rows(g, tile([cg, "7X"]), [cg, "7X"], 0)
        assert cg_fields(got) == [fused + "7X"]
        got, _ = run_rows(g, tile(["7X", cg]), ["7X", cg], 0)
        assert cg_fields(got) == ["7X" + fused]
        got, _ = run_rows(g, tile([cg, "7X"]), [cg, "7X"], -1)
        assert cg_fields(got) == [cg, "7X"]
    got, tally = run_rows(g, tile(["17=3I", "2I20="], gaps=[(2, 0)]), ["17=3I", "2I20="], 5)
    assert cg_fields(got) == ["17=7I20="] and tally["paf_joins_gap"] == 1
    got, _ = run_rows(g, tile(["17=3D", "2D20="], gaps=[(0, 4)]), ["17=3D", "2D20="], 5)
    assert cg_fields(got) == ["17=9D20="]
    got, _ = run_rows(g, tile(["17=3I", "2D20="], gaps=[(2, 4)]), ["17=3I", "2D20="], 5)
    assert cg_fields(got) == ["17=5I6D20="]
    got, _ = run_rows(g, tile(["17=3I", "2D20="], gaps=[(2, 4)]), ["17=3I", "2D20="], 3)  # (the gap is too wide: two lines)
    assert cg_fields(got) == ["17=3I", "2D20="]
    # the reverse strand: the later row in sorted order prints FIRST, the gap's ops between them
    rows = tile(["10=2D", "3D8=", "4=1X"], reverse=True, gaps=[(0, 3), (0, 0)])
    got, tally = run_rows(g, rows, ["10=2D", "3D8=", "4=1X"], 5)
    assert cg_fields(got) == ["10=8D12=1X"]  # 2D + the gap's 3D + 3D, 8= + 4=
    assert tally["reverse_multi_runs"] == 1 and tally["paf_joins_gap"] == 1 and tally["paf_joins_contiguous"] == 1
    assert got.split("\t")[4] == "-"


def test_digit_borders(plain):
    g = plain
    for a, b, want in (("4=", "6=", "10="), ("90=", "9=", "99="), ("99=", "1=", "100="), ("999999=", "1=", "1000000=")):
        got, _ = run_rows(g, tile([a, b]), [a, b], 0)
        assert cg_fields(got) == [want]
    big = (1 << 28) - 5  # one fused op of 2^28 bases: nine digits, on sequences below 2^29
    got, _ = run_rows(g, tile(["%d=" % big, "5="], q0=10, t0=20), ["%d=" % big, "5="], 0)
    assert cg_fields(got) == ["268435456="]
    line = got.split("\t")
    assert line[9] == line[10] == "268435456" and line[1] == line[6] == str((1 << 29) - 1)
    got, _ = run_rows(g, tile(["3=", "4="]), ["3=", "4="], 0, original_sequence_coordinates=True)
    assert got.split("\t")[1] == "0" and got.split("\t")[6] == "0"


@pytest.mark.parametrize("every", [0, 97])
def test_through_chains(plain, every):
    """5 000 one-op rows of one code on each strand, all contiguous: one op per run; at d = -1 they print raw.  With
    another code on every 97th row the groups end there.  No lane walks the chain: the suffix scan serves it."""
    g = plain
    n = 5000
    cigars = ["3X" if every and i % every == every - 1 else "3=" for i in range(n)]
    fwd = [(1, 3 * i, 3 * i + 3, 0, 3 * i, 3 * i + 3) for i in range(n)]
    rev = [(2, 3 * i + 3, 3 * i, 0, 3 * (n - i) - 3, 3 * (n - i)) for i in range(n)]
    got, tally = run_rows(g, fwd + rev, cigars + cigars, 0)
    assert got.count("\n") == 2 and tally["paf_joins_contiguous"] == 2 * (n - 1)
    if every:
        assert tally["paf_ops_printed"] == 2 * (2 * (n // every) + 1) and tally["reverse_through_rows"] > 4000
        assert cg_fields(got)[0].startswith("288=3X288=3X")
    else:
        assert cg_fields(got) == ["15000=", "15000="] and tally["paf_through_rows"] == 2 * (n - 1) and tally["paf_ops_printed"] == 2
    got, tally = run_rows(g, fwd + rev, cigars + cigars, -1)
    assert got.count("\n") == 2 * n and tally["paf_ops_printed"] == 2 * n and tally["paf_through_rows"] == 0


def refused(call, code, words):
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        call()
    assert ei.value.code == code and words in str(ei.value), str(ei.value)


def test_refused_rows(plain):
    """a target interval that runs backwards where the reference looks, a row without ops, a range without a row -- as the
    BEDPE entry refuses them; the next call answers"""
    g = plain
    eq = [ref.pack("20=")]
    a, b, back = (1, 10, 30, 0, 110, 130), (1, 30, 50, 0, 130, 150), (1, 50, 70, 0, 170, 150)

    def run(rows, rr, n_ranges, cigars, d):
        return g.selftest_paf_rows(np.array(rows, dtype=impg_amd.INTERVAL_DTYPE), rr, n_ranges, cigars, merge_distance=d,
                                   range_names=["x%d" % q for q in range(n_ranges)]).decode()

    good = [SELF_ROW, a, b]
    assert cg_fields(run(good, [0, 0, 0], 1, eq * 3, 0)) == ["40="]
    refused(lambda: run([SELF_ROW, a, back], [0, 0, 0], 1, eq * 3, 0), impg_amd.IMPG_E_INVALID, "Target intervals should always be in forward")
    assert run([SELF_ROW, a, back], [0, 0, 0], 1, eq * 3, -1).count("\n") == 2  # no merge: nobody looks
    refused(lambda: run(good, [0, 0, 0], 1, eq * 2 + [np.zeros(0, dtype=np.uint32)], 0), impg_amd.IMPG_E_UNSUPPORTED, "a result row without CIGAR")
    refused(lambda: run(good, [1, 1, 1], 2, eq * 3, 0), impg_amd.IMPG_E_INVALID, "no result row to drop")
    assert cg_fields(run(good, [0, 0, 0], 1, eq * 3, 0)) == ["40="]
    assert run([], [], 0, [], 0) == "" and g.counter("paf_rows") == 0


# ---- parameters, plumbing -----------------------------------------------------------------------------------------------
PARAMS = [dict(), dict(transitive=True, max_depth=2), dict(transitive=True, dfs=True, max_depth=3, min_transitive_len=50), dict(min_identity=0.7),
          dict(min_output_length=300)]


@pytest.mark.parametrize("seed,weird,incons,max_ops", [(91, False, False, 60), (92, True, False, 60), (93, True, True, 200),
                                                        (94, False, False, 12)])
def test_parameters_on_random_pafs(tmp_path, seed, weird, incons, max_ops):
    """The random PAFs of test_paf_and_bedpe_bytes (300 records, 60 ranges): plain, -x -m 2, DFS, min_identity and
    min_output_length at d = -1, 0, 25, 1000; a range the oracle refuses is refused by the device, alone in its batch;
    subset_keep."""
    sl = 30000
    text, names = random_paf(seed, 300, n_seq=5, seq_len=sl, max_ops=max_ops, weird=weird, inconsistent=incons, self_aln=True)
    g, c = both(tmp_path, "r.paf", text)
    ranges = random_ranges(seed, 60, 5, sl, max_len=6000, min_len=150)
    rnames = ["r%d" % i for i in range(len(ranges))]
    for kw in PARAMS:
        for d in (-1, 0, 25, 1000):
            want = {}
            for i, (t, s, e) in enumerate(ranges):
                try:
                    want[i] = c.query_paf(c.seq_name(t), s, e, range_name=rnames[i], merge_distance=d, fmt="paf", **kw)
                except RuntimeError:
                    want[i] = None
                    with pytest.raises(impg_amd.ImpgGpuError):
                        g.query_batch_paf([ranges[i]], impg_amd.make_params(**kw), merge_distance=d, range_names=[rnames[i]])
            live = [i for i in range(len(ranges)) if want[i] is not None]
            got = g.query_batch_paf([ranges[i] for i in live], impg_amd.make_params(**kw), merge_distance=d, range_names=[rnames[i] for i in live])
            assert got == "".join(want[i] for i in live), (kw, d)
            if d == 25:
                assert got == host_text(g, [ranges[i] for i in live], [rnames[i] for i in live], d, **kw), kw
    if weird or incons:
        return
    keep = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    kw = dict(transitive=True, max_depth=2)
    got = g.query_batch_paf(ranges, impg_amd.make_params(**kw), merge_distance=25, range_names=rnames, subset_keep=keep)
    assert got == host_text(g, ranges, rnames, 25, subset_keep=keep, **kw)
    assert got != g.query_batch_paf(ranges, impg_amd.make_params(**kw), merge_distance=25, range_names=rnames)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """an index whose names include "base:START-END" ones, 40 ranges, and the oracle's text for them at d = 50"""
    text, names = random_paf(95, 300, n_seq=5, seq_len=30000, max_ops=60, self_aln=True)
    for k, nm in enumerate(("s", "base:999-50000", "other:7-9", "L" * 200, "chrC:oops-5")):
        text = text.replace("s%d\t" % k, nm + "\t")
    tmp = tmp_path_factory.mktemp("paf_world")
    g, c = both(tmp, "w.paf", text)
    rl = random_ranges(9, 40, 5, 30000, max_len=4000, min_len=150)
    rnames = ["name%d" % i if i % 3 else "n" for i in range(len(rl))]
    kw = dict(transitive=True, max_depth=2)
    return g, c, rl, rnames, kw, oracle_text(c, rl, rnames, 50, **kw), str(tmp / "w.paf")


def test_chunks_and_pieces(world):
    g, c, rl, rnames, kw, want, _ = world
    p = impg_amd.make_params(**kw)
    assert g.query_batch_paf(rl, p, merge_distance=50, range_names=rnames) == want
    whole = counters(g)
    assert whole["paf_text_pieces"] == 1 and whole["paf_text_bytes"] == len(want.encode())
    try:
        for chunk in (1, 7):
            g.set_option("chunk_ranges", chunk)
            assert g.query_batch_paf(rl, p, merge_distance=50, range_names=rnames) == want, chunk
            have = counters(g)  # every chunk adds to the call's counters
            assert {k: have[k] for k in ref.COUNTERS} == {k: whole[k] for k in ref.COUNTERS}
            assert 2 <= have["paf_text_pieces"] <= -(-len(rl) // chunk)
        g.set_option("chunk_ranges", 0)
        longest = max(len(ln) + 1 for ln in want.splitlines())
        g.set_option("bed_text_piece_bytes", max(64, longest))  # lines fall into several pieces of whole lines
        assert g.query_batch_paf(rl, p, merge_distance=50, range_names=rnames) == want
        assert g.counter("paf_text_pieces") > 1 and g.counter("paf_text_bytes") == len(want.encode())
    finally:
        g.set_option("chunk_ranges", 0)
        g.set_option("bed_text_piece_bytes", 256 << 20)


def test_names_and_original_coordinates(world):
    g, c, rl, rnames, kw, want, _ = world
    p = impg_amd.make_params(**kw)
    made_up = ["%s:%d-%d" % (c.seq_name(t), s, e) for t, s, e in rl]
    assert g.query_batch_paf(rl, p, merge_distance=50) == oracle_text(c, rl, made_up, 50, **kw)
    okw = dict(original_sequence_coordinates=True, **kw)
    got = three_way(g, c, rl, rnames, 50, **okw)  # lengths 0, shifted names
    assert "base\t0\t" in got and "base:999" not in got and got != want


def test_fd_and_empty_batch(world):
    g, c, rl, rnames, kw, want, _ = world
    p = impg_amd.make_params(**kw)
    rd, wr = os.pipe()
    chunks = []

    def drain():
        with os.fdopen(rd, "rb") as f:
            chunks.append(f.read())

    th = threading.Thread(target=drain)
    th.start()
    try:
        n, sec = g.query_batch_paf(rl, p, merge_distance=50, range_names=rnames, fd=wr, timing=True)
    finally:
        os.close(wr)
        th.join()
    assert chunks[0].decode() == want and n == len(chunks[0]) and len(sec) == 3 and all(x >= 0 for x in sec)
    assert g.query_batch_paf([], p, merge_distance=50) == ""
    assert g.counter("paf_rows") == 0 and g.counter("paf_text_pieces") == 0


def test_refused_ranges(world):
    """a range with no row to drop: the code and message of the host route, no text; the handle goes on"""
    g, c, rl, rnames, kw, want, _ = world
    p = impg_amd.make_params(min_output_length=10 ** 8)
    with pytest.raises(RuntimeError):
        c.query_paf(c.seq_name(rl[0][0]), rl[0][1], rl[0][2], merge_distance=0, fmt="paf", min_output_length=10 ** 8)
    refused(lambda: g.query_batch_paf(rl[:1], p, merge_distance=0), impg_amd.IMPG_E_INVALID, "no result row to drop")
    by_len = sorted(rl, key=lambda r: r[2] - r[1])
    mixed, p = by_len[-5:] + by_len[:1], impg_amd.make_params(min_output_length=1000)
    g.set_option("chunk_ranges", 3)
    try:
        refused(lambda: g.query_batch_paf(mixed, p, merge_distance=0), impg_amd.IMPG_E_INVALID, "no result row to drop")
        assert g.query_batch_paf(mixed[:5], p, merge_distance=0, range_names=["x"] * 5) == oracle_text(c, mixed[:5], ["x"] * 5, 0, min_output_length=1000)
    finally:
        g.set_option("chunk_ranges", 0)
    assert g.query_batch_paf(rl, impg_amd.make_params(**kw), merge_distance=50, range_names=rnames) == want


def test_refused_handles(tmp_path):
    """handles the device route leaves to the host route: sharded and multi-GPU ones, a sequence of 2^29 bases or more, and
    -- where the host route refuses too -- a tracepoint index"""
    text, names = random_paf(96, 200, n_seq=4, seq_len=20000, max_ops=40, self_aln=True)
    path = write(tmp_path, "m.paf", text)
    rl = random_ranges(4, 10, 4, 20000, max_len=3000, min_len=150)
    m = impg_amd.GpuImpg.from_paf(path, devices=[0, 0], lanes=1)
    refused(lambda: m.query_batch_paf(rl, merge_distance=10), impg_amd.IMPG_E_UNSUPPORTED, "sharded")
    refused(lambda: m.query_batch_paf([], merge_distance=10), impg_amd.IMPG_E_UNSUPPORTED, "sharded")
    g = impg_amd.GpuImpg.from_paf(path)
    rnames = ["%s:%d-%d" % (g.seq_name(t), s, e) for t, s, e in rl]
    assert g.query_batch_paf(rl, merge_distance=10) == host_text(m, rl, rnames, 10) == host_text(g, rl, rnames, 10)
    rec, ops, sl = impg_amd.synth_paf(1, 500, n_seq=4, seq_len=100000, target_span=2000, n_blocks=10)
    for top, served in ((1 << 29, False), ((1 << 29) - 1, True)):
        sl2 = sl.copy()
        sl2[3] = top
        h = impg_amd.GpuImpg.from_records(rec, ops, sl2)
        ranges = random_ranges(5, 10, 3, 100000, max_len=5000, min_len=200)
        names = ["q%d" % i for i in range(len(ranges))]
        if served:
            assert h.query_batch_paf(ranges, merge_distance=10, range_names=names) == host_text(h, ranges, names, 10)
        else:
            refused(lambda: h.query_batch_paf(ranges, merge_distance=10, range_names=names), impg_amd.IMPG_E_UNSUPPORTED, "2^29")
    d = random_tp(3, 300, n_seq=5, seq_len=60000, fastga=True, self_aln=False)
    tp = impg_amd.GpuImpg.from_tracepoints(d["records"], d["tracepoints"], d["seq_len"], query_deltas=d["query_deltas"], diffs=d["diffs"],
                                           fastga=d["fastga"], trace_spacing=d["trace_spacing"], max_complexity=d["max_complexity"])
    tr = random_ranges(3, 5, 5, 60000, max_len=4000, min_len=101)
    for approx in (0, 1):
        tp.set_option("approximate_cigar", approx)
        refused(lambda: tp.query_batch_paf(tr, merge_distance=0), impg_amd.IMPG_E_UNSUPPORTED, "PAF output of approximate-mode results")
        refused(lambda: tp.query_batch_paf([], merge_distance=0), impg_amd.IMPG_E_UNSUPPORTED, "PAF output of approximate-mode results")
    p = impg_amd.make_params(store_cigar=True)
    refused(lambda: tp.query_batch(tr, p).paf(None, merge_distance=0, params=p, fmt="paf"), impg_amd.IMPG_E_UNSUPPORTED,
            "PAF output of approximate-mode results")


def test_cli_device_route_equals_host_merge(world):
    """`impg-gpu query -o paf` prints what `--host-merge` prints, byte for byte"""
    g, c, rl, rnames, kw, want, paf = world
    cli = os.path.join(os.path.dirname(impg_amd.__file__), "impg-gpu")
    bed = os.path.join(os.path.dirname(paf), "q.bed")
    with open(bed, "w") as f:
        for (t, s, e), rn in zip(rl[:12], rnames):
            f.write("%s\t%d\t%d\t%s\n" % (g.seq_name(t), s, e, rn))
    outs = []
    for extra in ([], ["--host-merge"]):
        r = subprocess.run([cli, "query", "-a", paf, "-b", bed, "-o", "paf", "-d", "50", "-x", "-m", "2"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1] and outs[0].count("\n") >= 12 and "\tcg:Z:" in outs[0]
