"""impg_gpu_query_batch_bedpe (impg_amd/csrc/bedpe_device.hip): query, CIGAR summaries, merge_adjusted_intervals and the
BEDPE text on the device.  Every comparison is three-way where the oracle can take part: device text == host route
(query_batch with store_cigar + .paf(fmt="bedpe")) == oracle; the counters against the model of tests/bedpe_ref.py, which
tests/test_bedpe_ref_cpu.py holds against the oracle.  Every case is small."""
import os
import threading

import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import bedpe_ref as ref
from tests.paf_gen import random_paf, random_ranges
from tests.tp_gen import random_tp

pytestmark = pytest.mark.gpu

GROUP = 4  # lanes per row of the summary kernel: 2 ** (option "bedpe_group_log2", by default)
COUNTER_KEYS = ref.COUNTERS + ("bedpe_text_pieces",)


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
    return g.query_batch(ranges, p, subset_keep=subset_keep).paf(rnames, merge_distance=d, params=p, fmt="bedpe")


def oracle_text(c, ranges, rnames, d, **kw):
    return "".join(c.query_paf(c.seq_name(t), s, e, range_name=rn, merge_distance=d, fmt="bedpe", **kw) for (t, s, e), rn in zip(ranges, rnames))


def three_way(g, c, ranges, rnames, d, **kw):
    got = g.query_batch_bedpe(ranges, impg_amd.make_params(**kw), merge_distance=d, range_names=rnames)
    assert got == oracle_text(c, ranges, rnames, d, **kw), (d, kw)
    assert got == host_text(g, ranges, rnames, d, **kw), (d, kw)
    return got


def model_counters(c, ranges, rnames, d, **kw):
    tally = ref.new_counters()
    for (t, s, e), rn in zip(ranges, rnames):
        rows, cigars = c.query_cigar(t, s, e, **kw)
        rows = [(r["query_id"], r["q_first"], r["q_last"], r["target_id"], r["t_first"], r["t_last"]) for r in rows]
        ref.bedpe_range(rows, cigars, d, rn, c.seq_name, transitive=bool(kw.get("transitive")), counters=tally)
    return tally


# ---- dense sets -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    """20 dense tilings side by side in one index (their sequences told apart by a prefix) and all their ranges"""
    texts, ranges = [], []
    for seed in range(20):
        text, rs = ref.dense_paf(seed, prefix="k%d_" % seed)
        texts.append(text)
        ranges.append((seed, rs))
    g, c = both(tmp_path_factory.mktemp("bedpe_dense"), "dense.paf", "".join(texts))
    rl = [(g.seq_id("k%d_%s" % (seed, ref.DENSE_NAMES[t])), s, e) for seed, rs in ranges for (t, s, e) in rs]
    assert all(g.seq_name(t) == c.seq_name(t) for t, _, _ in rl)
    return g, c, rl, ["r%d" % i for i in range(len(rl))]


@pytest.mark.parametrize("d", [-1, 0, 1, 2, 5, 100])
def test_dense_sets(dense, d):
    """60 ranges over tilings whose blocks lie 0, 1, 2, 5 or -1 bases apart, in one call: the text three ways, and the
    counters are the model's sums -- both join kinds, fusing at joins and inside rows, both strands ran."""
    g, c, rl, rnames = dense
    got = three_way(g, c, rl, rnames, d)
    want = model_counters(c, rl, rnames, d)
    have = counters(g)
    assert {k: have[k] for k in ref.COUNTERS} == {k: want[k] for k in ref.COUNTERS}
    assert have["bedpe_text_bytes"] == len(got) and have["bedpe_text_pieces"] == 1
    if d >= 5:
        assert want["bedpe_joins_contiguous"] >= 50 and want["bedpe_joins_gap"] >= 50 and want["joins_reverse"] >= 50
        assert want["fused_at_joins"] >= 20 and want["fused_in_rows"] >= 20
    if d < 0:
        assert have["bedpe_runs"] == have["bedpe_rows"] and have["bedpe_fused_ops"] == 0


# ---- summary kernel edges ---------------------------------------------------------------------------------------------
def cigar_of(rng, n_ops):
    """n_ops random ops, neighbours of one kind allowed (I-I and D-D pairs fuse once the row is joined)"""
    return "".join("%d%s" % (int(rng.integers(1, 9)), "=XID"[int(rng.integers(0, 4))]) for _ in range(n_ops))


def test_summary_kernel_edges(tmp_path):
    """CIGARs of 1, 2, G-1, G, G+1, 2G+1 and 1000 ops (and the same around 16 and 64 lanes, the widest group), each as two
    contiguous records that join at d = 0, covered whole; a range inside one op; a range clipping the first and the last
    op; a CIGAR ending in I and one starting with D on either side of a gap join; a 3D-only row (q_first == q_last).
    Every group width prints the same text."""
    rng = np.random.default_rng(7)
    lines, ranges = [], []
    tpos, qpos = 1000, 500
    for n_ops in (1, 2, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1, 15, 16, 17, 33, 63, 64, 65, 129, 1000):
        start = tpos
        for _ in range(2):
            cg = cigar_of(rng, n_ops)
            td, qd = ref.cigar_spans(cg)
            if td == 0 or qd == 0:
                cg += "7="
                td, qd = td + 7, qd + 7
            lines.append("Q\t400000\t%d\t%d\t+\tT\t400000\t%d\t%d\t1\t1\t60\tcg:Z:%s" % (qpos, qpos + qd, tpos, tpos + td, cg))
            tpos, qpos = tpos + td, qpos + qd
        ranges.append((start, tpos))
        tpos, qpos = tpos + 500, qpos + 700
    a = tpos  # one long op; a CIGAR whose first and last op a range clips
    lines.append("Q\t400000\t%d\t%d\t+\tT\t400000\t%d\t%d\t1\t1\t60\tcg:Z:600=" % (qpos, qpos + 600, a, a + 600))
    ranges += [(a + 200, a + 320), (a - 50, a + 650)]
    b = a + 2000
    lines.append("Q\t400000\t%d\t%d\t-\tT\t400000\t%d\t%d\t1\t1\t60\tcg:Z:40=5X30=3I30=2D40=" % (qpos + 5000, qpos + 5148, b, b + 147))
    ranges += [(b + 10, b + 140), (b + 39, b + 41)]
    e = b + 2000  # ... 17=3I | one base on the target | 2D18=: the gap's D between an I and a D
    lines.append("Q\t400000\t%d\t%d\t+\tT\t400000\t%d\t%d\t1\t1\t60\tcg:Z:17=3I" % (qpos + 9000, qpos + 9020, e, e + 17))
    lines.append("Q\t400000\t%d\t%d\t+\tT\t400000\t%d\t%d\t1\t1\t60\tcg:Z:2D18=" % (qpos + 9020, qpos + 9038, e + 18, e + 38))
    lines.append("Q\t400000\t%d\t%d\t+\tT\t400000\t%d\t%d\t1\t1\t60\tcg:Z:3D" % (qpos + 9038, qpos + 9038, e + 38, e + 41))
    lines.append("Q\t400000\t%d\t%d\t+\tT\t400000\t%d\t%d\t1\t1\t60\tcg:Z:2I20=" % (qpos + 9038, qpos + 9060, e + 41, e + 61))
    ranges += [(e - 5, e + 70)]
    g, c = both(tmp_path, "edges.paf", "\n".join(lines) + "\n", bidirectional=False)
    t = g.seq_id("T")
    rl = [(t, s, x) for s, x in ranges]
    rnames = ["e%d" % i for i in range(len(rl))]
    for d in (-1, 0, 5):
        three_way(g, c, rl, rnames, d, min_transitive_len=1)  # (the reference takes no range shorter than that, whatever the query)
        n_ops = sum(len(cg) for (_, s, x) in rl for cg in c.query_cigar(t, s, x)[1][1:])
        assert g.counter("bedpe_summary_ops") == n_ops and n_ops > 2400
    assert g.counter("bedpe_joins_contiguous") >= 15 and g.counter("bedpe_joins_gap") >= 1 and g.counter("bedpe_fused_ops") >= 1
    want = g.query_batch_bedpe(rl, merge_distance=5, range_names=rnames)
    for lg in (3, 4, 5, 6, 2):  # 8 .. 64 lanes a row, and back to the default
        g.set_option("bedpe_group_log2", lg)
        assert g.query_batch_bedpe(rl, merge_distance=5, range_names=rnames) == want, lg
        assert g.counter("bedpe_summary_ops") == n_ops


# ---- random sets ------------------------------------------------------------------------------------------------------
PARAMS = [dict(), dict(transitive=True, max_depth=2), dict(transitive=True, dfs=True, max_depth=3, min_transitive_len=50), dict(min_identity=0.7),
          dict(min_output_length=300)]


@pytest.mark.parametrize("seed,weird,incons,max_ops", [(91, False, False, 60), (92, True, False, 60), (93, True, True, 200),
                                                        (94, False, False, 12)])
def test_random_sets(tmp_path, seed, weird, incons, max_ops):
    """The indexes of test_paf_and_bedpe_bytes (tests/test_gpu_parity.py): plain, -x -m 2, DFS -m 3, min_identity and
    min_output_length at d = -1, 0, 25, 1000.  A range the oracle refuses is refused by the device, alone in its batch."""
    sl = 30000
    text, names = random_paf(seed, 300, n_seq=5, seq_len=sl, max_ops=max_ops, weird=weird, inconsistent=incons, self_aln=True)
    g, c = both(tmp_path, "r.paf", text)
    ranges = random_ranges(seed, 60, 5, sl, max_len=6000, min_len=150)[:24]
    rnames = ["r%d" % i for i in range(len(ranges))]
    for kw in PARAMS:
        want = {}
        for d in (-1, 0, 25, 1000):
            for i, (t, s, e) in enumerate(ranges):
                try:
                    want[(d, i)] = c.query_paf(c.seq_name(t), s, e, range_name=rnames[i], merge_distance=d, fmt="bedpe", **kw)
                except RuntimeError:
                    want[(d, i)] = None
                    with pytest.raises(impg_amd.ImpgGpuError):
                        g.query_batch_bedpe([ranges[i]], impg_amd.make_params(**kw), merge_distance=d, range_names=[rnames[i]])
            live = [i for i in range(len(ranges)) if want[(d, i)] is not None]
            got = g.query_batch_bedpe([ranges[i] for i in live], impg_amd.make_params(**kw), merge_distance=d, range_names=[rnames[i] for i in live])
            assert got == "".join(want[(d, i)] for i in live), (kw, d)
            if d == 25:
                assert got == host_text(g, [ranges[i] for i in live], [rnames[i] for i in live], d, **kw), kw


# ---- plumbing ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """an index whose names include "base:START-END" ones, 40 ranges, and the oracle's text for them at d = 50"""
    text, names = random_paf(95, 300, n_seq=5, seq_len=30000, max_ops=60, self_aln=True)
    for k, nm in enumerate(("s", "base:999-50000", "other:7-9", "L" * 200, "chrC:oops-5")):
        text = text.replace("s%d\t" % k, nm + "\t")
    g, c = both(tmp_path_factory.mktemp("bedpe_world"), "w.paf", text)
    rl = random_ranges(9, 40, 5, 30000, max_len=4000, min_len=150)
    rnames = ["name%d" % i if i % 3 else "n" for i in range(len(rl))]
    kw = dict(transitive=True, max_depth=2)
    return g, c, rl, rnames, kw, oracle_text(c, rl, rnames, 50, **kw)


def test_chunks_and_pieces(world):
    g, c, rl, rnames, kw, want = world
    p = impg_amd.make_params(**kw)
    assert g.query_batch_bedpe(rl, p, merge_distance=50, range_names=rnames) == want
    whole = counters(g)
    assert whole["bedpe_text_pieces"] == 1 and whole["bedpe_text_bytes"] == len(want.encode())
    try:
        for chunk in (1, 7):
            g.set_option("chunk_ranges", chunk)
            assert g.query_batch_bedpe(rl, p, merge_distance=50, range_names=rnames) == want, chunk
            have = counters(g)  # every chunk adds to the call's counters
            assert {k: have[k] for k in ref.COUNTERS} == {k: whole[k] for k in ref.COUNTERS}
            assert 2 <= have["bedpe_text_pieces"] <= -(-len(rl) // chunk)  # (a chunk without a line sends no piece)
        g.set_option("chunk_ranges", 0)
        g.set_option("bed_text_piece_bytes", 64)  # its lowest value: a piece per line, the long name's lines included
        assert g.query_batch_bedpe(rl, p, merge_distance=50, range_names=rnames) == want
        assert g.counter("bedpe_text_pieces") == want.count("\n") > 1 and g.counter("bedpe_text_bytes") == len(want.encode())
    finally:
        g.set_option("chunk_ranges", 0)
        g.set_option("bed_text_piece_bytes", 256 << 20)


def test_names_and_coordinates(world):
    g, c, rl, rnames, kw, want = world
    p = impg_amd.make_params(**kw)
    made_up = ["%s:%d-%d" % (c.seq_name(t), s, e) for t, s, e in rl]
    assert g.query_batch_bedpe(rl, p, merge_distance=50) == oracle_text(c, rl, made_up, 50, **kw)
    mixed = [None if i % 2 else rnames[i] for i in range(len(rl))]
    assert g.query_batch_bedpe(rl, p, merge_distance=50, range_names=mixed) == oracle_text(
        c, rl, [made_up[i] if i % 2 else rnames[i] for i in range(len(rl))], 50, **kw)
    okw = dict(original_sequence_coordinates=True, **kw)
    got = three_way(g, c, rl, rnames, 50, **okw)
    assert "base\t" in got and "base:999" not in got and got != want


def test_nameless_index_and_subset():
    rec, ops, sl = impg_amd.synth_paf(1, 3000, n_seq=6, seq_len=100000, target_span=2000, n_blocks=10)
    g = impg_amd.GpuImpg.from_records(rec, ops, sl)
    assert g.seq_name(0) is None
    rl = random_ranges(3, 30, 6, 100000, max_len=5000, min_len=200)
    rnames = ["q%d" % i for i in range(len(rl))]
    for kw in (dict(), dict(transitive=True, max_depth=2)):
        got = g.query_batch_bedpe(rl, impg_amd.make_params(**kw), merge_distance=100, range_names=rnames)
        assert got == host_text(g, rl, rnames, 100, **kw) and got.count("\n") > len(rl)
        assert g.query_batch_bedpe(rl, impg_amd.make_params(**kw), merge_distance=100) == host_text(g, rl, None, 100, **kw)  # "{id}:{start}-{end}"
    keep = np.array([1, 0, 1, 1, 0, 1], dtype=np.uint8)
    kw = dict(transitive=True, max_depth=2)
    got = g.query_batch_bedpe(rl, impg_amd.make_params(**kw), merge_distance=100, range_names=rnames, subset_keep=keep)
    assert got == host_text(g, rl, rnames, 100, subset_keep=keep, **kw)
    assert got != g.query_batch_bedpe(rl, impg_amd.make_params(**kw), merge_distance=100, range_names=rnames)


def test_fd_and_empty_batch(world):
    g, c, rl, rnames, kw, want = world
    p = impg_amd.make_params(**kw)
    rd, wr = os.pipe()
    chunks = []

    def drain():
        with os.fdopen(rd, "rb") as f:
            chunks.append(f.read())

    th = threading.Thread(target=drain)
    th.start()
    try:
        n, sec = g.query_batch_bedpe(rl, p, merge_distance=50, range_names=rnames, fd=wr, timing=True)
    finally:
        os.close(wr)
        th.join()
    assert chunks[0].decode() == want and n == len(chunks[0]) and len(sec) == 3 and all(x >= 0 for x in sec)
    text, sec = g.query_batch_bedpe(rl, p, merge_distance=50, range_names=rnames, timing=True)
    assert text == want and len(sec) == 3 and sec[0] > 0 and sec[1] > 0 and sec[2] > 0
    assert g.query_batch_bedpe([], p, merge_distance=50) == ""
    assert g.counter("bedpe_rows") == 0 and g.counter("bedpe_text_pieces") == 0


# ---- refusals ---------------------------------------------------------------------------------------------------------
def refused(call, code, words):
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        call()
    assert ei.value.code == code and words in str(ei.value), str(ei.value)


def test_refused_ranges(world):
    """a batch that holds only the error: the code and message of the host route, no text; the handle goes on"""
    g, c, rl, rnames, kw, want = world
    # every row of a plain query fails the retain: nothing to drop (the reference panics in Vec::remove(0))
    p = impg_amd.make_params(min_output_length=10 ** 8)
    with pytest.raises(RuntimeError):
        c.query_paf(c.seq_name(rl[0][0]), rl[0][1], rl[0][2], merge_distance=0, fmt="bedpe", min_output_length=10 ** 8)
    refused(lambda: g.query_batch_bedpe(rl[:1], p, merge_distance=0), impg_amd.IMPG_E_INVALID, "no result row to drop")
    refused(lambda: g.query_batch(rl[:1], impg_amd.make_params(store_cigar=True, min_output_length=10 ** 8)).paf(
        None, merge_distance=0, params=p, fmt="bedpe"), impg_amd.IMPG_E_INVALID, "no result row to drop")
    # ... also as the last range of the second chunk: the first chunk's text is not returned either
    by_len = sorted(rl, key=lambda r: r[2] - r[1])
    mixed, p = by_len[-5:] + by_len[:1], impg_amd.make_params(min_output_length=1000)
    assert oracle_text(c, mixed[:5], ["x"] * 5, 0, min_output_length=1000).count("\n") >= 5
    with pytest.raises(RuntimeError):
        oracle_text(c, mixed[5:], ["x"], 0, min_output_length=1000)
    g.set_option("chunk_ranges", 3)
    try:
        refused(lambda: g.query_batch_bedpe(mixed, p, merge_distance=0), impg_amd.IMPG_E_INVALID, "no result row to drop")
        assert g.query_batch_bedpe(mixed[:5], p, merge_distance=0, range_names=["x"] * 5) == oracle_text(c, mixed[:5], ["x"] * 5, 0, min_output_length=1000)
    finally:
        g.set_option("chunk_ranges", 0)
    assert g.query_batch_bedpe(rl, impg_amd.make_params(**kw), merge_distance=50, range_names=rnames) == want


def iv(qid, qf, ql, tid, tf, tl):
    return (qid, qf, ql, tid, tf, tl)


def test_refused_rows(world):
    """the merge on rows of our own (impg_gpu_selftest_bedpe_rows): the refusals no query of these indexes reaches -- a
    target interval that runs backwards, exactly where the reference looks at it -- and the two it does, each alone"""
    g = world[0]
    eq = [np.array([20], dtype=np.uint32)]  # 20=
    self_row = iv(0, 100, 200, 0, 100, 200)
    a, b, back = iv(1, 10, 30, 0, 110, 130), iv(1, 30, 50, 0, 130, 150), iv(1, 50, 70, 0, 170, 150)

    def run(rows, rr, n_ranges, cigars, d):
        return g.bedpe_rows(np.array(rows, dtype=impg_amd.INTERVAL_DTYPE), rr, n_ranges, cigars, merge_distance=d,
                            range_names=["x%d" % q for q in range(n_ranges)]).decode()

    def model(rows, cigars, d, name):
        return ref.bedpe_range(rows, cigars, d, name, g.seq_name, transitive=True)

    good = [self_row, a, b]
    assert run(good, [0, 0, 0], 1, eq * 3, 0) == model(good, eq * 3, 0, "x0") and g.counter("bedpe_joins_contiguous") == 1
    # two rows or more after the drop and d >= 0: the reference looks at every row's target
    rows = [self_row, a, back]
    with pytest.raises(ref.Refused):
        model(rows, eq * 3, 0, "x0")
    refused(lambda: run(rows, [0, 0, 0], 1, eq * 3, 0), impg_amd.IMPG_E_INVALID, "Target intervals should always be in forward")
    refused(lambda: run([self_row, back, a], [0, 0, 0], 1, eq * 3, 1000), impg_amd.IMPG_E_INVALID, "Target intervals should always be in forward")
    assert run(rows, [0, 0, 0], 1, eq * 3, -1) == model(rows, eq * 3, -1, "x0")  # no merge: nobody looks
    assert run([self_row, back], [0, 0], 1, eq * 2, 0) == model([self_row, back], eq * 2, 0, "x0")  # a single row: the fold is not entered
    # ... in the second range of two, with a good first one
    two = good + rows
    refused(lambda: run(two, [0, 0, 0, 1, 1, 1], 2, eq * 6, 0), impg_amd.IMPG_E_INVALID, "Target intervals should always be in forward")
    assert run(two, [0, 0, 0, 1, 1, 1], 2, eq * 6, -1) == model(good, eq * 3, -1, "x0") + model(rows, eq * 3, -1, "x1")
    # a row without ops; a range without a row
    none = [np.zeros(0, dtype=np.uint32)]
    refused(lambda: run(good, [0, 0, 0], 1, eq * 2 + none, 0), impg_amd.IMPG_E_UNSUPPORTED, "a result row without CIGAR")
    assert run(good, [0, 0, 0], 1, none + eq * 2, 0) == model(good, eq * 3, 0, "x0")  # (the dropped row's ops are never read)
    refused(lambda: run(good, [1, 1, 1], 2, eq * 3, 0), impg_amd.IMPG_E_INVALID, "no result row to drop")
    refused(lambda: run(good, [0, 0, 0], 2, eq * 3, 0), impg_amd.IMPG_E_INVALID, "no result row to drop")
    assert run(good, [0, 0, 0], 1, eq * 3, 0) == model(good, eq * 3, 0, "x0")
    assert run([], [], 0, [], 0) == ""


@pytest.mark.parametrize("d", [-1, 0])
def test_sort_guard_edges(world, d):
    """where the order's guards stand, on rows of our own: no row left after the drop (no text), exactly one left (no
    sort), and 257 left -- one more than a block of threads -- that tie on every key of all three passes, so that only
    emission order tells them apart: the text and the counters are the model's"""
    g = world[0]
    rng = np.random.default_rng(258)
    self_row = iv(0, 100, 200, 0, 100, 200)

    def row(ln):  # same sequences, strand, q start and t_first; the ends and the ops differ: "a= bX c="
        a, b = (int(x) for x in rng.integers(0, ln + 1, 2))
        a, b = min(a, b), max(a, b) - min(a, b)
        ops = [n | code << 29 for n, code in ((a, 0), (b, 1), (ln - a - b, 0)) if n]
        return iv(1, 10, 10 + ln, 0, 110, 110 + ln), np.array(ops, dtype=np.uint32)

    tied = [row(int(ln)) for ln in rng.integers(1, 60, 257)]
    assert any(x[0][2] > y[0][2] for x, y in zip(tied, tied[1:]))  # (no key would have put them in this order)
    eq = np.array([100], dtype=np.uint32)
    cases = [([[self_row]] * 3, [[eq]] * 3, 0),
             ([[self_row, tied[0][0]]], [[eq, tied[0][1]]], 1),
             ([[self_row] + [r for r, _ in tied]], [[eq] + [c for _, c in tied]], 257)]
    for rows, cigars, left in cases:
        names = ["x%d" % q for q in range(len(rows))]
        tally = ref.new_counters()
        want = "".join(ref.bedpe_range(r, c, d, nm, g.seq_name, transitive=True, counters=tally) for r, c, nm in zip(rows, cigars, names))
        flat = np.array([x for r in rows for x in r], dtype=impg_amd.INTERVAL_DTYPE)
        rr = [q for q, r in enumerate(rows) for _ in r]
        got = g.bedpe_rows(flat, rr, len(rows), [x for c in cigars for x in c], merge_distance=d, range_names=names).decode()
        assert got == want and got.count("\n") == left, (d, left)
        have = counters(g)
        assert {k: have[k] for k in ref.COUNTERS} == {k: tally[k] for k in ref.COUNTERS}, (d, left)
        assert have["bedpe_rows"] == left == have["bedpe_runs"] and have["bedpe_text_pieces"] == (1 if left else 0)


def test_refused_handles(tmp_path):
    """handles the device route leaves to the host route: sharded and multi-GPU ones, a sequence of 2^29 bases or more"""
    text, names = random_paf(96, 200, n_seq=4, seq_len=20000, max_ops=40, self_aln=True)
    path = write(tmp_path, "m.paf", text)
    rl = random_ranges(4, 10, 4, 20000, max_len=3000, min_len=150)
    m = impg_amd.GpuImpg.from_paf(path, devices=[0, 0], lanes=1)
    refused(lambda: m.query_batch_bedpe(rl, merge_distance=10), impg_amd.IMPG_E_UNSUPPORTED, "sharded")
    refused(lambda: m.query_batch_bedpe([], merge_distance=10), impg_amd.IMPG_E_UNSUPPORTED, "sharded")
    g = impg_amd.GpuImpg.from_paf(path)
    rnames = ["%s:%d-%d" % (g.seq_name(t), s, e) for t, s, e in rl]
    want = g.query_batch_bedpe(rl, merge_distance=10)
    assert want == host_text(m, rl, rnames, 10) == host_text(g, rl, rnames, 10)  # (the multi handle's host route goes on)
    rec, ops, sl = impg_amd.synth_paf(1, 500, n_seq=4, seq_len=100000, target_span=2000, n_blocks=10)
    for top, served in ((1 << 29, False), ((1 << 29) - 1, True)):
        sl2 = sl.copy()
        sl2[3] = top
        h = impg_amd.GpuImpg.from_records(rec, ops, sl2)
        ranges = random_ranges(5, 10, 3, 100000, max_len=5000, min_len=200)
        names = ["q%d" % i for i in range(len(ranges))]
        if served:
            assert h.query_batch_bedpe(ranges, merge_distance=10, range_names=names) == host_text(h, ranges, names, 10)
        else:
            refused(lambda: h.query_batch_bedpe(ranges, merge_distance=10, range_names=names), impg_amd.IMPG_E_UNSUPPORTED, "2^29")
            assert host_text(h, ranges, names, 10).count("\n") >= len(ranges)


# ---- tracepoint index -------------------------------------------------------------------------------------------------
def test_tracepoint_index():
    """approximate mode: the two-count CIGARs through the same summaries and merge; a 0-op row is refused as on the host"""
    d = random_tp(3, 700, n_seq=5, seq_len=60000, fastga=True, self_aln=False)
    g = impg_amd.GpuImpg.from_tracepoints(d["records"], d["tracepoints"], d["seq_len"], query_deltas=d["query_deltas"], diffs=d["diffs"],
                                          fastga=d["fastga"], trace_spacing=d["trace_spacing"], max_complexity=d["max_complexity"])
    ranges = random_ranges(3, 60, 5, 60000, max_len=4000, min_len=101)
    rnames = ["t%d" % i for i in range(len(ranges))]
    refused(lambda: g.query_batch_bedpe(ranges[:2], merge_distance=0), impg_amd.IMPG_E_UNSUPPORTED, "approximate_cigar")
    refused(lambda: g.query_batch_bedpe([], merge_distance=0), impg_amd.IMPG_E_UNSUPPORTED, "approximate_cigar")
    g.set_option("approximate_cigar", 1)
    no_ops = 0
    for kw in (dict(), dict(transitive=True, max_depth=2, min_transitive_len=30), dict(transitive=True, max_depth=3, min_transitive_len=30)):
        p = impg_amd.make_params(store_cigar=True, **kw)
        res = g.query_batch(ranges, p)
        live = []
        for i in range(len(ranges)):
            if any(len(cg) == 0 for cg in res.cigars(i)[1:]):
                no_ops += 1
                if no_ops <= 3:  # alone in its batch: the host route's code and message
                    refused(lambda: g.query_batch_bedpe([ranges[i]], impg_amd.make_params(**kw), merge_distance=0), impg_amd.IMPG_E_UNSUPPORTED,
                            "a result row without CIGAR")
                    refused(lambda: g.query_batch([ranges[i]], p).paf([rnames[i]], merge_distance=0, params=p, fmt="bedpe"),
                            impg_amd.IMPG_E_UNSUPPORTED, "a result row without CIGAR")
            else:
                live.append(i)
        assert len(live) > len(ranges) // 2
        for dist in (-1, 0, 1000):
            got = g.query_batch_bedpe([ranges[i] for i in live], impg_amd.make_params(**kw), merge_distance=dist, range_names=[rnames[i] for i in live])
            assert got == host_text(g, [ranges[i] for i in live], [rnames[i] for i in live], dist, **kw), (kw, dist)
            assert got.count("\n") >= len(live)
    assert no_ops >= 1
