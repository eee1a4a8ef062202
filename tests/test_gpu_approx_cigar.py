"""store_cigar on a tracepoint index (option approximate_cigar): the approximate mode's CIGAR, and the BEDPE text made of it.

project_overlapping_interval_fast returns, beside the coordinates, the pair the identity filter is computed from:
[round(total_matches) '='] if positive, then [round(total_mismatches) 'X'] if positive (impg.rs:1479-1486) -- 0, 1 or 2 ops
that are counts, not an alignment.  With the option set every store_cigar entry point returns them; here rows and ops are
compared with the oracle's own restatement (OracleIndex.query_cigar / query_paf on a tracepoint index) over the shapes of
tests/test_gpu_parity.py::test_tracepoint_approximate_mode: 700 alignments, 5 sequences of 60 000 bp, Standard and FASTGA.

Two things the oracle's interface decides for these tests:
  * query_cigar takes neither a mask nor a subset filter.  For those two runs the rows come from OracleIndex.query (which
    takes both) and every row's ops from the plain query_cigar of the row's own target interval: the approximate CIGAR of a
    hit depends on the alignment and on the target stretch that is projected, and a transitive hit projects the clipped
    stretch it reports as t_first..t_last (impg.rs:2398-2400), which lies inside the alignment, so Impg::query on that
    stretch scans the same segments.  expected_ops() is first checked against query_cigar's own BFS answer.
  * a tracepoint index is created without sequence names and prints ids where the oracle prints the names it made up
    ("seq3"); the oracle's BEDPE columns 1 and 4 are mapped through its own name -> id table before the texts are compared.
"""
import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests.paf_gen import random_ranges
from tests.tp_gen import random_tp

pytestmark = pytest.mark.gpu

CASES = [(False, 1), (False, 2), (True, 3), (True, 4)]
N_SEQ, SEQ_LEN = 5, 60_000
BFS = dict(transitive=True, max_depth=3, min_transitive_len=30)
# BEDPE: the depth-3 closure of the FASTGA seeds reaches a 0-op row -- which the oracle does not print -- from 15 % of seed
# 3's ranges (oracle alone, on the CPU); at depth 2 it is one range of 120, inside the 5 % the text test allows
BFS_TEXT = dict(transitive=True, max_depth=2, min_transitive_len=30)
_fix, _ref = {}, {}


def tp_index(d, **kw):
    return impg_amd.GpuImpg.from_tracepoints(d["records"], d["tracepoints"], d["seq_len"], query_deltas=d["query_deltas"], diffs=d["diffs"],
                                             fastga=d["fastga"], trace_spacing=d["trace_spacing"], max_complexity=d["max_complexity"], **kw)


def fixture(fastga, seed):
    """(input arrays, engine index with the option set, oracle index, 120 ranges of 101..4000 bp), one per case."""
    if seed not in _fix:
        d = random_tp(seed, 700, n_seq=N_SEQ, seq_len=SEQ_LEN, fastga=fastga, self_aln=(seed % 2 == 0))
        g = tp_index(d)
        g.set_option("approximate_cigar", 1)
        _fix[seed] = (d, g, o.OracleIndex(tracepoints=d), random_ranges(seed, 120, N_SEQ, SEQ_LEN, max_len=4000, min_len=101))
    return _fix[seed]


def reference(seed, c, ranges, **kw):
    """[(rows, [ops])] of the oracle for `ranges`, computed once per (seed, query kind) and left unchanged."""
    key = (seed, len(ranges), tuple(sorted(kw.items())))
    if key not in _ref:
        _ref[key] = [c.query_cigar(t, s, e, **kw) for (t, s, e) in ranges]
    return _ref[key]


def op_classes(ref):
    """the kinds of rows in an oracle answer, by their op letters: (), ('=',), ('X',), ('=', 'X'); self rows left out"""
    kinds = {}
    for rows, cg in ref:
        for ops in cg[1:]:
            k = tuple("=XIDM"[int(x) >> 29] for x in ops)
            kinds[k] = kinds.get(k, 0) + 1
    return kinds


def same_as(res, ref, what):
    for i, (want, wcg) in enumerate(ref):
        assert res[i].tolist() == want.tolist(), (what, i)
        assert [x.tolist() for x in res.cigars(i)] == [x.tolist() for x in wcg], (what, i)


def check(g, seed, c, ranges, **kw):
    res = g.query_batch(ranges, impg_amd.make_params(store_cigar=True, **kw))
    same_as(res, reference(seed, c, ranges, **kw), kw)
    return res


def expected_ops(c, row, cache):
    """every op list Impg::query gives a row with `row`'s six fields when asked for the row's own target interval"""
    q, qf, ql, t, tf, tl = row
    if tf >= tl:
        return None  # (no range to ask with)
    key = (t, tf, tl)
    if key not in cache:
        rows, cg = c.query_cigar(t, tf, tl)
        cache[key] = {}
        for r, ops in zip(rows.tolist(), cg):
            cache[key].setdefault(tuple(r), set()).add(tuple(ops.tolist()))
    return cache[key].get(tuple(row), set())


def same_by_rows(res, c, want_rows, cache, what):
    """rows against OracleIndex.query's; ops against expected_ops (equal where one alignment gives the row, else one of them)"""
    n_one = n_all = 0
    for i, want in enumerate(want_rows):
        assert res[i].tolist() == want.tolist(), (what, i)
        for row, ops in zip(want.tolist(), res.cigars(i)):
            cand = expected_ops(c, row, cache)
            if cand is None:
                continue
            assert tuple(ops.tolist()) in cand, (what, i, row)
            n_all += 1
            n_one += len(cand) == 1
    assert n_all and n_one >= 0.99 * n_all, (what, n_one, n_all)  # (rows two alignments give with different ops are rare)


def random_mask(seed, n_seq, seq_len, max_ranges=8):
    """{seq id: (sequence_length, sorted disjoint non-touching ranges)}: a masked_regions map"""
    rng = np.random.default_rng(seed)
    mask = {}
    for sid in range(n_seq):
        if rng.random() > 0.8:
            continue
        cuts = np.unique(rng.integers(0, seq_len, size=2 * int(rng.integers(0, max_ranges + 1))))
        cuts = cuts[: 2 * (len(cuts) // 2)]
        mask[sid] = (seq_len, [(int(cuts[2 * i]), int(cuts[2 * i + 1])) for i in range(len(cuts) // 2)])
    return mask


@pytest.mark.parametrize("fastga,seed", CASES)
def test_cigar_parity(fastga, seed):
    """Rows and ops of every store_cigar query kind equal the oracle's: plain, BFS, BFS under the identity filter (one pair
    of sums feeds the filter and the ops), DFS, MultiImpg (the five-key sort permutes the slots, ops included), a masked BFS
    and subset-filtered runs (dropped slots write no ops)."""
    d, g, c, ranges = fixture(fastga, seed)
    plain, bfs = reference(seed, c, ranges), reference(seed, c, ranges[:60], **BFS)
    kinds = op_classes(plain + bfs)
    # the inputs hold the kinds of rows the oracle alone finds in them (a Standard segment always has max_complexity or
    # max(qd, t) mismatches: no '='-only and no 0-op row there -- test_every_row_kind_by_hand has all four in one index)
    assert kinds.get(("=", "X"), 0) > 1000 and kinds.get(("X",), 0) > 10, kinds
    if fastga:
        assert kinds.get(("=",), 0) > 10 and kinds.get((), 0) > 0, kinds
    assert set(kinds) <= {(), ("=",), ("X",), ("=", "X")}
    before = g.counter("project_tp_levels")
    check(g, seed, c, ranges)
    assert g.counter("project_tp_levels") == before + 1  # (the tracepoint kernel's levels are still counted)
    check(g, seed, c, ranges[:60], **BFS)
    check(g, seed, c, ranges[:60], min_identity=0.8, **BFS)
    check(g, seed, c, ranges[:40], transitive=True, dfs=True, max_depth=2, min_transitive_len=50)
    check(g, seed, c, ranges[:40], multi_impg=True)
    check(g, seed, c, ranges[:40], transitive=True, max_depth=2, multi_impg=True, min_transitive_len=50)
    # the trait-shaped calls answer too (the rows; a batch of one range has the ops)
    t0, s0, e0 = ranges[0]
    assert g.query(t0, s0, e0, store_cigar=True, approximate_mode=True).tolist() == plain[0][0].tolist()
    assert g.query_transitive_bfs(t0, s0, e0, max_depth=3, min_transitive_len=30, store_cigar=True,
                                  approximate_mode=True).tolist() == bfs[0][0].tolist()
    kw = dict(transitive=True, dfs=True, max_depth=2, min_transitive_len=50)
    assert g.query_transitive_dfs(t0, s0, e0, max_depth=2, min_transitive_len=50, store_cigar=True,
                                  approximate_mode=True).tolist() == reference(seed, c, ranges[:40], **kw)[0][0].tolist()
    # mask and subset filter: rows from OracleIndex.query, ops row by row (module docstring); the row-by-row reference first
    # has to reproduce query_cigar's own BFS answer
    cache = {}
    for rows, cg in bfs[:20]:
        for row, ops in zip(rows.tolist(), cg):
            cand = expected_ops(c, row, cache)
            assert cand is None or tuple(ops.tolist()) in cand, row
    mask = random_mask(seed * 10 + 1, N_SEQ, SEQ_LEN)
    res = g.query_batch(ranges[:30], impg_amd.make_params(store_cigar=True, **BFS), masked_regions=mask)
    same_by_rows(res, c, [c.query(t, s, e, masked_regions=mask, **BFS) for (t, s, e) in ranges[:30]], cache, "masked")
    keep = (np.random.default_rng(seed).random(N_SEQ) < 0.5).astype(np.uint8)
    for kw in (dict(), BFS):
        res = g.query_batch(ranges[:30], impg_amd.make_params(store_cigar=True, **kw), subset_keep=keep)
        want = [c.query(t, s, e, subset_keep=keep, **kw) for (t, s, e) in ranges[:30]]
        full = reference(seed, c, ranges if not kw else ranges[:60], **kw)[:30]
        assert sum(len(w) for w in want) < sum(len(rows) for rows, _ in full)  # (the filter drops rows)
        same_by_rows(res, c, want, cache, ("subset", kw))


@pytest.mark.parametrize("strand", [0, 1])
def test_every_row_kind_by_hand(strand):
    """One FASTGA alignment of four segments (trace spacing 100; target deltas 100, 0, 0, 100; diffs 0, 0, 5, 7), target
    1000-1200 of sequence 1, query 5000-5400 of sequence 0: its segments have 100 matches / no mismatch, neither (an
    insertion without diffs), 5 mismatches only, and 93 / 7 -- so ranges over single segments and over all of them give
    a '='-only, a 0-op, an 'X'-only and a two-op row (worked from impg.rs:771-802, :1479-1486; the oracle agrees)."""
    rec = np.zeros(1, dtype=o.TP_RECORD_DTYPE)
    rec[0] = (0, 1, 5000, 5400, 1000, 1200, 0, 4, strand, 0)
    d = dict(records=rec, tracepoints=np.array([100, 0, 0, 100], dtype=np.int32), query_deltas=None,
             diffs=np.array([0, 0, 5, 7], dtype=np.int32), fastga=True, trace_spacing=100, max_complexity=0,
             seq_len=np.array([10000, 10000], dtype=np.int64))
    g, c = tp_index(d), o.OracleIndex(tracepoints=d)
    g.set_option("approximate_cigar", 1)
    # on the query axis (the reversed entry) the four segments are 5000-5100, .. , 5300-5400 whatever the strand
    ranges = [(0, 5000, 5100), (0, 5100, 5110), (0, 5100, 5200), (0, 5200, 5300), (0, 5300, 5400), (0, 5100, 5300), (0, 4900, 5500),
              (1, 900, 1300), (1, 1000, 1010), (1, 1100, 1110), (1, 1190, 1200), (1, 1050, 1150)]
    ref = [c.query_cigar(t, s, e) for (t, s, e) in ranges]
    kinds = op_classes(ref)
    assert set(kinds) == {(), ("=",), ("X",), ("=", "X")}, kinds
    E, X = 0 << 29, 1 << 29
    assert [ref[k][1][1].tolist() for k in (0, 1, 3, 4, 6)] == [[100 | E], [], [5 | X], [93 | E, 7 | X], [193 | E, 12 | X]]
    same_as(g.query_batch(ranges, impg_amd.make_params(store_cigar=True)), ref, "by hand")
    kw = dict(transitive=True, max_depth=2, min_transitive_len=1)
    same_as(g.query_batch(ranges, impg_amd.make_params(store_cigar=True, **kw)), [c.query_cigar(t, s, e, **kw) for (t, s, e) in ranges], kw)


@pytest.mark.parametrize("fastga,seed", CASES)
def test_sharded(fastga, seed):
    """The same alignments sharded over three ranks of one handle, two lanes, chunks of 11 ranges: the owner materialises
    the ops (Engine::expand) and they follow the hits home; the option set on the handle reaches every rank's engine."""
    d, g, c, ranges = fixture(fastga, seed)
    gm = tp_index(d, devices=[0, 0, 0], lanes=2)
    gm.set_option("chunk_ranges", 11)
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        gm.query_batch(ranges[:3], impg_amd.make_params(store_cigar=True))
    assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED
    gm.set_option("approximate_cigar", 1)
    check(gm, seed, c, ranges)
    check(gm, seed, c, ranges[:60], **BFS)
    # ... and the text of what came home
    want, shown = bedpe_reference(seed, c, ranges, **BFS_TEXT)
    rs = [ranges[i] for i in shown]
    res = gm.query_batch(rs, impg_amd.make_params(store_cigar=True, **BFS_TEXT))
    assert res.paf([range_name(c, r) for r in rs], merge_distance=1000, params=impg_amd.make_params(store_cigar=True, **BFS_TEXT),
                   fmt="bedpe") == "".join(want[1000][i] for i in shown)


@pytest.mark.parametrize("fastga,seed", CASES[1:3])
def test_stream(fastga, seed):
    """impg_gpu_query_batch_stream with store_cigar: 120 ranges in chunks of 16 deliver the rows and ops of query_batch."""
    d, g, c, ranges = fixture(fastga, seed)
    for kw in (dict(), BFS):
        p = impg_amd.make_params(store_cigar=True, **kw)
        whole = g.query_batch(ranges, p)
        got, firsts = {}, []

        def consumer(first, part):
            firsts.append(first)
            for k in range(len(part)):
                got[first + k] = (part[k].tolist(), [x.tolist() for x in part.cigars(k)])
            return 0

        g.query_batch_stream(ranges, consumer, params=p, chunk_ranges=16, copy=True)
        assert firsts == list(range(0, 120, 16)) and sorted(got) == list(range(120))
        for i in range(120):
            assert got[i] == (whole[i].tolist(), [x.tolist() for x in whole.cigars(i)]), (kw, i)
        same_as(whole, reference(seed, c, ranges if not kw else ranges[:60], **kw), kw)  # (and query_batch itself is the oracle's answer)


def range_name(c, r):
    return "%s:%d-%d" % (c.seq_name(r[0]), r[1], r[2])


def bedpe_reference(seed, c, ranges, **kw):
    """({merge distance: [text per range, None where the oracle refuses the range]}, the ranges it prints), once per
    (seed, query kind).  The oracle refuses a range that holds a 0-op row ("empty CIGAR in a BEDPE row": the reference's
    gap-2d merge of such a range is not restated); columns 1 and 4 are mapped from its names to ids (module docstring)."""
    key = ("bedpe", seed, len(ranges), tuple(sorted(kw.items())))
    if key not in _ref:
        ids = {c.seq_name(i): str(i) for i in range(c.num_seqs())}
        texts = {}
        for dist in (-1, 0, 1000):
            texts[dist] = []
            for r in ranges:
                try:
                    text = c.query_paf(c.seq_name(r[0]), r[1], r[2], range_name=range_name(c, r), merge_distance=dist, fmt="bedpe", **kw)
                except RuntimeError as ex:
                    assert "empty CIGAR in a BEDPE row" in str(ex), ex
                    texts[dist].append(None)
                    continue
                lines = []
                for line in text.splitlines():
                    f = line.split("\t")
                    f[0], f[3] = ids[f[0]], ids[f[3]]
                    lines.append("\t".join(f) + "\n")
                texts[dist].append("".join(lines))
        shown = [i for i, t in enumerate(texts[-1]) if t is not None]
        assert all([i for i, t in enumerate(texts[dist]) if t is not None] == shown for dist in texts)
        assert len(ranges) - len(shown) <= 0.05 * len(ranges), (len(shown), len(ranges))  # (or the test would compare next to nothing)
        _ref[key] = (texts, shown)
    return _ref[key]


@pytest.mark.parametrize("fastga,seed", CASES)
def test_bedpe_text(fastga, seed):
    """impg_gpu_results_paf(IMPG_OUT_BEDPE) on approximate results: byte for byte what the oracle prints for `impg query
    --approximate -o bedpe` (merge_adjusted_intervals on the two-count CIGARs, gi / bi from them; main.rs:11894-11987), for
    no merge, distance 0 and distance 1000, plain and BFS; a batch holding a range with a 0-op row is refused."""
    d, g, c, ranges = fixture(fastga, seed)
    n_changed = 0
    for kw in (dict(), BFS_TEXT):
        want, shown = bedpe_reference(seed, c, ranges, **kw)
        rs = [ranges[i] for i in shown]
        p = impg_amd.make_params(store_cigar=True, **kw)
        res = g.query_batch(rs, p)
        names = [range_name(c, r) for r in rs]
        for dist in (-1, 0, 1000):
            assert res.paf(names, merge_distance=dist, params=p, fmt="bedpe") == "".join(want[dist][i] for i in shown), (kw, dist)
        n_changed += sum(want[-1][i].count("\n") != want[1000][i].count("\n") for i in shown)
        with pytest.raises(impg_amd.ImpgGpuError) as ei:  # the reference refuses paf in approximate mode (main.rs:7387-7397)
            res.paf(names, merge_distance=0, params=p, fmt="paf")
        assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED
        hidden = [i for i in range(len(ranges)) if i not in shown]
        if hidden:  # a range the oracle does not print: the batch holding it is refused as a whole, its ops are the oracle's
            rs = [ranges[shown[0]], ranges[hidden[0]]]
            res = g.query_batch(rs, p)
            with pytest.raises(impg_amd.ImpgGpuError) as ei:
                res.paf([range_name(c, r) for r in rs], merge_distance=0, params=p, fmt="bedpe")
            assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED
            rows, cg = c.query_cigar(*ranges[hidden[0]], **kw)
            assert res[1].tolist() == rows.tolist() and [x.tolist() for x in res.cigars(1)] == [x.tolist() for x in cg]
            assert any(len(x) == 0 for x in cg[1:])
    assert n_changed > 10  # (merging at distance 1000 joins rows in these inputs: the merge arms ran)


def test_op_longer_than_29_bits():
    """A sum of 2^29 or more does not fit a CigarOp: CigarOp::new panics in the reference (impg.rs:88), here the run ends
    with IMPG_E_INVALID and no truncated op is returned.  One Standard alignment whose first segment spans 600 000 000 bases
    on both axes: any range inside that segment has 599 999 997 matches, whatever its own length.  (The oracle packs the
    length without the check, so only the rows and the ranges that fit are compared with it.)"""
    L = 600_000_000
    rec = np.zeros(1, dtype=o.TP_RECORD_DTYPE)
    rec[0] = (0, 1, 1000, 1000 + L + 100, 2000, 2000 + L + 100, 0, 2, 0, 0)
    d = dict(records=rec, tracepoints=np.array([L, 100], dtype=np.int32), query_deltas=np.array([L, 100], dtype=np.int32), diffs=None,
             fastga=False, trace_spacing=0, max_complexity=3, seq_len=np.array([L + 10_000, L + 10_000], dtype=np.int64))
    g, c = tp_index(d), o.OracleIndex(tracepoints=d)
    g.set_option("approximate_cigar", 1)
    long_op, fits = (1, 3000, 4000), (1, 2000 + L, 2000 + L + 50)
    assert L - 3 >= 1 << 29 and c.query(*long_op)[1].tolist() == (0, 2000, 3000, 1, 3000, 4000)
    assert g.query_batch([long_op, fits], impg_amd.make_params())[0].tolist() == c.query(*long_op).tolist()  # (rows alone: no op, no error)
    for rs in ([long_op], [fits, long_op]):
        for kw in (dict(), dict(transitive=True, max_depth=1, min_transitive_len=10)):
            with pytest.raises(impg_amd.ImpgGpuError) as ei:
                g.query_batch(rs, impg_amd.make_params(store_cigar=True, **kw))
            assert ei.value.code == impg_amd.IMPG_E_INVALID and "29 bits" in str(ei.value)
    res = g.query_batch([fits], impg_amd.make_params(store_cigar=True))  # (the engine answers again after the failed runs)
    same_as(res, [c.query_cigar(*fits)], "fits")
    assert [x.tolist() for x in res.cigars(0)] == [[50], [97, 3 | (1 << 29)]]


def test_refusals(tmp_path):
    """Without the option store_cigar on a tracepoint index stays IMPG_E_UNSUPPORTED, and the message names the option; the
    option takes 0 or 1; on a CIGAR index it is accepted and changes nothing."""
    from tests.paf_gen import random_paf
    d = random_tp(2, 700, n_seq=N_SEQ, seq_len=SEQ_LEN, fastga=False, self_aln=True)
    g = tp_index(d)
    ranges = random_ranges(2, 8, N_SEQ, SEQ_LEN, max_len=4000, min_len=101)
    for kw in (dict(), BFS, dict(transitive=True, dfs=True, max_depth=2), dict(multi_impg=True)):
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            g.query_batch(ranges, impg_amd.make_params(store_cigar=True, **kw))
        assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED and "approximate_cigar" in str(ei.value)
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        g.query_batch_stream(ranges, lambda first, part: 0, params=impg_amd.make_params(store_cigar=True), chunk_ranges=4)
    assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED
    with pytest.raises(impg_amd.ImpgGpuError):
        g.set_option("approximate_cigar", 2)
    g.set_option("approximate_cigar", 1)
    assert g.query_batch(ranges, impg_amd.make_params(store_cigar=True)).cigar_off is not None
    g.set_option("approximate_cigar", 0)  # (and off again)
    with pytest.raises(impg_amd.ImpgGpuError):
        g.query_batch(ranges, impg_amd.make_params(store_cigar=True))
    # rows in HBM stay without CIGARs, option or not
    g.set_option("approximate_cigar", 1)
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        g.query_batch_device(ranges, impg_amd.make_params(store_cigar=True))
    assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED
    # a CIGAR index: the option is accepted, its slices are the exact ones and print as PAF
    text, _ = random_paf(11, 200, n_seq=5, seq_len=30_000, self_aln=True)
    path = str(tmp_path / "x.paf")
    with open(path, "w") as f:
        f.write(text)
    gp, cp = impg_amd.GpuImpg.from_paf(path), o.OracleIndex(paf_paths=[path])
    gp.set_option("approximate_cigar", 1)
    rs = random_ranges(5, 40, 5, 30_000, max_len=3000, min_len=120)
    for kw in (dict(), dict(transitive=True, max_depth=2, min_transitive_len=40)):
        p = impg_amd.make_params(store_cigar=True, **kw)
        res = gp.query_batch(rs, p)
        same_as(res, [cp.query_cigar(t, s, e, **kw) for (t, s, e) in rs], kw)
        names = ["%s:%d-%d" % (cp.seq_name(t), s, e) for (t, s, e) in rs]
        assert res.paf(names, merge_distance=10, params=p, fmt="paf") == "".join(
            cp.query_paf(cp.seq_name(t), s, e, range_name=names[i], merge_distance=10, fmt="paf", **kw) for i, (t, s, e) in enumerate(rs))
