"""The lookup's wide-window paths at their edges, against the oracle -- and proof that each one ran.

A window of more than 64 entries (counted from its aligned start) leaves the lane kernels: lookup_count_wide_kernel counts
it and lookup_emit_wide_kernel emits it -- in one LDS pass, in groups of rank bins once it holds more hits than the key
buffer, or not at all when one bin alone overflows the buffer (the overflow list, lookup_emit_kernel); a fused final level
reads the same windows again in project_entries_kernel.  tests/lookup_gen.py builds the fixtures and says, from a plain
model, which path every window of a case takes; here each case runs with lookup_stats 1 in every result form, rows and
order against the oracle, under both lookup orders (locality_min 1 / 4096), fused and listed final levels, plain and
transitive, and the lookup_wide_* counters of every single run must rise by exactly what the model names -- so a window that
lands on another path, or a counter that stops counting, fails instead of passing on the wrong path (that the model's sums make
each of the five counters rise is tests/test_lookup_gen_cpu.py's check).  Options wide_emit_cap /
wide_emit_bins lower the two limits so that many-group windows and the overflow list are reached by a 1000-entry index."""
import pytest

import impg_amd
from oracle import oracle as o
from tests import lookup_gen as lg
from tests.proj_worker import FORMS, check_forms

pytestmark = pytest.mark.gpu

assert (lg.COITREES, lg.SORTED) == (impg_amd.ORDER_COITREES, impg_amd.ORDER_SORTED)
_built = {}


def built(case, tmp_path_factory):
    """(engine index, oracle index, {target: ranks}) of a case's fixture, one per (n, n2, order policy)."""
    key = (case.n, case.n2, case.order)
    if key not in _built:
        path = str(tmp_path_factory.mktemp("lk") / "l.paf")
        with open(path, "w") as f:
            f.write(lg.paf(case.n, case.n2))
        g = impg_amd.GpuImpg.from_paf(path, bidirectional=False, order=case.order)
        c = o.OracleIndex(paf_paths=[path], bidirectional=False, preparse=True)
        assert [g.seq_name(i) for i in range(g.num_seqs())] == [c.seq_name(i) for i in range(c.num_seqs())]
        m = len(lg.umbrella_entries(case.n2)) if case.n2 else 0
        assert g.num_entries() == case.n + m  # (the empty entries are entries: they hold ranks and widen windows)
        ranks = {}
        if case.order == lg.COITREES:
            if case.n:
                ranks["T"] = lg.visit_ranks(c, c.seq_id("T"), case.n)
            if m:  # (a segment's ranks are a function of its size: lookup_gen, "where a rank comes from")
                c2 = o.OracleIndex(paf_text=lg.paf(m), bidirectional=False, preparse=True)
                ranks["T2"] = lg.visit_ranks(c2, c2.seq_id("T"), m)
        g.set_option("walk_kernel", 0)  # (the per-query walk has a lookup of its own: every run here is the batch engine's)
        g.set_option("lookup_stats", 1)
        _built[key] = (g, c, ranks)
    return _built[key]


def snapshot(g):
    return {k: g.counter(k) for k in lg.COUNTERS}


@pytest.mark.parametrize("name", list(lg.CASES))
def test_lookup_path(tmp_path_factory, name):
    case = lg.CASES[name]
    g, c, ranks = built(case, tmp_path_factory)
    ranges = [(g.seq_id(t), s, e) for t, s, e in case.ranges]
    forms = case.forms or FORMS
    combos = lg.BOTH[:1] if name == "small_batch" else lg.BOTH  # (run_small has no lookup order and no fused level)
    small0 = g.counter("small_batches")
    if name == "small_batch":  # Engine::run_small takes it: plain, <= 64 ranges, their targets' segments sum to <= 2^18 entries
        assert len(ranges) <= lg.SMALL_RANGES and sum(case.n for _ in ranges) <= lg.SMALL_PAIRS and g.num_entries() == case.n
    if case.order == lg.SORTED:
        o.set_sorted_visits(True)
    try:
        cache, answers, overflowed = {}, {}, 0
        for cap, bins in case.limits:
            g.set_option("wide_emit_cap", cap)
            g.set_option("wide_emit_bins", bins)
            for lm, fuse in combos:
                g.set_option("locality_min", lm)
                g.set_option("fuse_final_level", fuse)
                for kw in case.modes:
                    plans, _ = lg.plans(case, ranks, bool(kw.get("transitive")), cap, bins)
                    want = lg.counters_of(plans)  # (a deeper level finds nothing: the query sequences own no entries)
                    for form in forms:
                        tag = (name, cap, bins, lm, fuse)
                        before = snapshot(g)
                        arms = check_forms(g, c, ranges, kw, forms=(form,), cache=cache, tag=tag)
                        after = snapshot(g)
                        got = {k: after[k] - before[k] for k in lg.COUNTERS}
                        assert got == want, (tag, kw, form)
                        overflowed += got["lookup_wide_overflow"]
                        if name == "fused_t2" and (lm, fuse) == (1, 1) and form in ("stats", "attributed"):
                            # a dense fused level: project_entries_kernel reads the wide windows (and their empty entries) itself
                            assert any(k.startswith("project_entries_") and v > 0 for k, v in arms[form].items()), (tag, kw, form, arms)
                    if "stats" in forms:  # the same counts and checksums at every setting of the two limits
                        st, cnt, ck = g.query_batch_stats(ranges, impg_amd.make_params(**kw))
                        key = (lm, fuse, tuple(sorted(kw.items())))
                        here = (int(st.projected), cnt.tolist(), ck.tolist())
                        assert answers.setdefault(key, here) == here, (name, cap, bins, key)
        if name == "small_batch":  # ... and did take it: every query_batch here was answered by the small-batch path
            assert g.counter("small_batches") - small0 == len(case.limits) * len(combos) * len(case.modes) * len(forms)
        if len(case.limits) > 1:  # the lowered limits reached the overflow list (and the defaults did not need it)
            assert overflowed > 0
    finally:
        o.set_sorted_visits(False)
        g.set_option("wide_emit_cap", lg.WIDE_CAP)
        g.set_option("wide_emit_bins", lg.WIDE_BINS)
        g.set_option("locality_min", 4096)
        g.set_option("fuse_final_level", 1)


def test_limits_out_of_range_are_refused_and_stats_off_counts_nothing(tmp_path):
    path = str(tmp_path / "l.paf")
    with open(path, "w") as f:
        f.write(lg.paf(200))
    g = impg_amd.GpuImpg.from_paf(path, bidirectional=False)
    for key, bad in (("wide_emit_cap", (63, 4097, 0, -1)), ("wide_emit_bins", (1, 1025, 0, -1))):
        for v in bad:
            with pytest.raises(impg_amd.ImpgGpuError) as e:
                g.set_option(key, v)
            assert e.value.code == impg_amd.IMPG_E_INVALID
    for key, ok in (("wide_emit_cap", (64, 4096)), ("wide_emit_bins", (2, 1024))):
        for v in ok:
            g.set_option(key, v)
    g.set_option("walk_kernel", 0)
    ranges = [(g.seq_id("T"),) + lg.ladder_range(0, 200)] * 3
    g.query_batch(ranges, impg_amd.make_params())
    g.query_batch_stats(ranges, impg_amd.make_params(**lg.M1))
    assert snapshot(g) == dict.fromkeys(lg.COUNTERS, 0)  # without the option a query leaves every lookup_wide_* counter where it was
    g.set_option("lookup_stats", 1)
    g.query_batch_stats(ranges, impg_amd.make_params(**lg.M1))
    assert snapshot(g) == dict(lookup_wide_windows=3, lookup_wide_single=3, lookup_wide_grouped=0, lookup_wide_group_passes=0, lookup_wide_overflow=0)
