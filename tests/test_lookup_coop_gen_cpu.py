"""tests/lookup_coop_gen.py on the CPU: the plain model against the oracle where the two can meet (sequence ids, segment
order, windows' hits), and that the cases as a whole reach every path and edge tests/test_gpu_lookup_coop.py is there for --
so a case that stops reaching its path fails here, not silently on the GPU."""
import pytest

from oracle import oracle as o
from tests import lookup_coop_gen as cg
from tests import lookup_gen as lg

FIXTURES = {c.fixture.name: c.fixture for c in cg.CASES.values()}


def paths(case, batch, transitive, span=cg.CAP):
    return cg.wave_paths(cg.layout(case.fixture), batch, transitive, span)[0]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_layout_and_hit_counts_match_the_oracle(name):
    fx = FIXTURES[name]
    lay = cg.layout(fx)
    c = o.OracleIndex(paf_text=cg.paf(fx), bidirectional=False, preparse=True)
    assert c.num_seqs() == lay.n_seq
    assert {c.seq_name(i): i for i in range(c.num_seqs())} == lay.ids
    assert all(c.seq_len(lay.ids[t]) == lay.seg[t][2] for t in lay.seg)
    # the model's hit count of a half-open window is the number of entries the oracle projects; a closed window holds at least those
    seen = 0
    for case in cg.CASES.values():
        if case.fixture is not fx:
            continue
        for batch in case.batches:
            for kw in (dict(), cg.M1):
                uniq = sorted({r for r in batch if r[0] != cg.BAD})[::7]
                win = cg.windows(lay, uniq, bool(kw))
                for (t, s, e), (_, _, hits) in zip(uniq, win):
                    c.query(lay.ids[t], s, e, **kw)
                    # (the closed test's window also holds entries that only touch the range and entries of length zero: candidates
                    # the oracle does not project)
                    n_proj = c.last_projection_count()
                    assert n_proj == hits if kw else n_proj <= hits, (case.name, t, s, e, kw)
                    seen += 1
    assert seen > 10


def test_batch_sizes_fill_whole_and_partial_waves():
    case = cg.CASES["batch_sizes"]
    assert [len(b) for b in case.batches] == list(cg.BATCH_SIZES) == [1, 63, 64, 65, 255, 256, 257, 320]
    for b in case.batches:
        for tr in (False, True):
            p = paths(case, b, tr)
            assert len(p) == (len(b) + 63) // 64 and set(p) == {"coop"}


def test_target_boundaries():
    case = cg.CASES["target_boundary"]
    lay = cg.layout(case.fixture)
    want = [["mixed"]] * 7 + [["coop", "coop"]]
    for b, w in zip(case.batches, want):
        for tr in (False, True):
            assert paths(case, b, tr) == w
    # where the odd range sits in its wave
    lanes = []
    for b in case.batches[:5]:
        order = cg.lookup_order(lay, b)
        first = b[order[0]][0]
        lanes.append([k for k, i in enumerate(order) if b[i][0] != first])
    assert lanes[0] == list(range(1, 64)) and lanes[1] == list(range(32, 64)) and lanes[2] == [63]
    assert lanes[3] == list(range(1, 64)) and b[order[0]][0] == cg.BAD  # the unknown target sorts first: key 0
    assert lay.seg["q0"][1] == 0 and {t for t, _, _ in case.batches[5]} == {"q0"}


def test_segment_sizes_reach_every_search_shape():
    case = cg.CASES["segment_sizes"]
    assert cg.SIZES == (1, 63, 64, 65, 127, 128, 4095, 4096, 4097)
    assert [cg.search_shape(n) for n in cg.SIZES] == ["block"] * 3 + ["samples"] * 6  # (1, 2, 2, 64, 64, 65 samples: one counting round)
    lay = cg.layout(case.fixture)
    assert len({lay.seg["S%d" % n][0] & 3 for n in cg.SIZES}) >= 3  # segments start on and off the vector boundary
    for n, b in zip(cg.SIZES, case.batches):
        for tr in (False, True):
            p = paths(case, b, tr)
            assert set(p) == {"coop"} and len(p) >= (3 if n > 100 else 1), (n, p)
        ub = [w[1] - lay.seg["S%d" % n][0] for w in cg.windows(lay, b, True)]
        assert max(ub) == n and min(w[0] for w in cg.windows(lay, b, True)) == lay.seg["S%d" % n][0]  # first and last entry reached


def test_narrowing_reaches_its_edges():
    """the kernel's own search shapes: 256 samples in one counting round, 257 and more narrowed first"""
    case = cg.CASES["narrowing"]
    lay = cg.layout(case.fixture)
    assert [cg.search_shape(n) for n in cg.NARROW_SIZES] == ["samples", "samples", "narrow", "narrow", "narrow"]
    assert [(n + 63) // 64 for n in cg.NARROW_SIZES] == [256, 256, 257, 257, 313]
    for n, b in zip(cg.NARROW_SIZES, case.batches):
        a, _, _, ent = lay.seg["N%d" % n]
        for tr in (False, True):
            p, waves = cg.wave_paths(lay, b, tr)
            assert p == ["coop"] * 4, (n, p)
            if cg.search_shape(n) != "narrow":
                continue
            rounds = []
            for w in waves:  # the three thresholds of every wave: l1(min end), l1(max end), l2(min start)
                rs = [b[i] for i in w]
                firsts = (cg.l1(ent, min(e for _, _, e in rs), tr), cg.l1(ent, max(e for _, _, e in rs), tr), cg.l2(ent, min(s for _, s, _ in rs), tr))
                rounds += [cg.narrow_trace(n, f) for f in firsts]
            assert all(len(r) == 1 for r in rounds)                           # one narrowing round, then <= 256 samples remain
            steps = {r[0][0] for r in rounds}
            assert steps == {5}                                               # ceil(257 / 64) = ceil(313 / 64) = 5: a rounded step
            assert all(r[0][1] > 0 for r in rounds)                           # probes beyond the last sample, clamped to it
            ks = {r[0][2] for r in rounds}
            assert None in ks and 0 in ks and max(k for k in ks if k is not None) >= (n + 63) // 64 // 5 - 1  # no probe passes; first; last
            assert any(k not in (None, 0) and k < 40 for k in ks)            # ... and a middle one
        win = cg.windows(lay, b, True)
        assert min(lo for lo, _, _ in win) == a and max(ub for _, ub, _ in win) == a + n


def test_span_limit_edges():
    case = cg.CASES["span_limit"]
    lay = cg.layout(case.fixture)
    assert case.spans == (8, 64, cg.CAP) and cg.SPAN_WIDTHS == (8, 9, 64, 65, cg.CAP, cg.CAP + 1)
    for tr in (False, True):
        for w, b in zip(cg.SPAN_WIDTHS, case.batches):
            assert len(b) == 64
            _, S0, S1 = cg.wave_path(lay, b, tr)
            assert S1 - S0 == w
            for span in case.spans:
                assert paths(case, b, tr, span) == ["coop" if w <= span else "span"]


def test_reductions_sit_in_the_lanes_they_are_meant_for():
    case = cg.CASES["reductions"]
    lay = cg.layout(case.fixture)
    (b,) = case.batches
    assert cg.lookup_order(lay, b) == list(range(64)) and len({cg.order_key(lay, *r[:2]) for r in b}) == 1
    starts, ends = [s for _, s, _ in b], [e for _, _, e in b]
    assert starts.index(min(starts)) == 63 and ends.index(min(ends)) == 20 and ends.index(max(ends)) == 40
    assert max(ends) > lay.seg["R"][3][-1][1]  # behind the segment's last end
    assert paths(case, b, False) == paths(case, b, True) == ["coop"]


def test_window_positions_and_comparison_edges():
    lay = cg.layout(cg.FX_R)
    a, n, _, ent = lay.seg["R"]
    assert a & 3 and n == 100
    pos = cg.CASES["window_positions"].batches[0]
    for tr in (False, True):
        win = cg.windows(lay, pos, tr)
        assert any(lo == ub == a for lo, ub, _ in win)              # before the first entry
        assert any(lo == ub == a + n for lo, ub, _ in win)          # behind the last end
        assert any(a < lo == ub < a + n for lo, ub, _ in win)       # a gap: l2 = l1
        assert any(lo < ub and lo & 3 for lo, ub, _ in win)         # a window that begins off the vector boundary
        assert any(s == 0 for _, s, _ in pos)
        assert set(paths(cg.CASES["window_positions"], pos, tr)) == {"coop"}
    edge = cg.CASES["comparison_edges"].batches[0]
    starts = {s for s, _ in ent}
    pm, run = set(), None
    for _, e in ent:
        run = e if run is None else max(run, e)
        pm.add(run)
    assert any(e in starts for _, _, e in edge) and any(s in pm for _, s, _ in edge)
    assert any(s == e for s, e in ent)  # INT_MIN in ends_t
    # the two tests differ on these ranges: the edges are edges
    assert cg.windows(lay, edge, False) != cg.windows(lay, edge, True)
    assert set(paths(cg.CASES["comparison_edges"], edge, False)) == {"coop"}


def test_wide_rule_inside_a_cooperative_wave():
    case = cg.CASES["wide_rule"]
    lay = cg.layout(case.fixture)
    (b,) = case.batches
    assert lay.seg["A"][0] == 0 and len(b) == 64
    for tr in (False, True):
        assert paths(case, b, tr) == ["coop"]
        widths = sorted(ub - (lo & ~3) for lo, ub, _ in cg.windows(lay, b, tr) if ub - (lo & ~3) >= 64)
        assert widths == [64, 64, 65, 65, 67, 68]
        assert cg.counters_of(lay, b, tr)["lookup_wide_windows"] == 4


def test_every_counter_rises_somewhere():
    total = dict.fromkeys(cg.COUNTERS + ("lookup_wide_windows",), 0)
    for case in cg.CASES.values():
        lay = cg.layout(case.fixture)
        for b in case.batches:
            for span in case.spans:
                for k, v in cg.counters_of(lay, b, True, span).items():
                    if k in total:
                        total[k] += v
    assert all(v > 0 for v in total.values()), total
    lay = cg.layout(cg.FX_AB)
    assert not any(cg.counters_of(lay, cg.CASES["batch_sizes"].batches[-1], True, coop=False)[k] for k in cg.COUNTERS)
