"""The cooperative count kernel at its edges, against the oracle -- and proof of the path every wave took.

Under a lookup order (locality_min 1) a level's ranges are counted by lookup_count_coop_kernel: a wave searches once for its
64 ranges, copies the span of the index columns they need into LDS and lets every lane finish there -- or, when its ranges
name more than one target, an unknown or an empty one, or span more than lookup_coop_span entries, takes the lane kernel's
body.  tests/lookup_coop_gen.py builds the fixtures and says, from a plain model, which path every wave of a batch takes;
here every batch runs with lookup_stats 1 in every result form, rows and order against the oracle, plain and transitive,
fused and listed final level, with lookup_coop 1 and 0, and the three wave counters of every single run must rise by exactly
what the model names (by nothing with lookup_coop 0, and on the small-batch path, which has no lookup order) while the
lookup_wide_* counters rise by the same amounts under both settings.  That the cases reach what they are there for is
tests/test_lookup_coop_gen_cpu.py's check."""
import pytest

import impg_amd
from oracle import oracle as o
from tests import lookup_coop_gen as cg
from tests import lookup_gen as lg
from tests.paf_gen import random_paf, random_ranges
from tests.proj_worker import FORMS, check_forms

pytestmark = pytest.mark.gpu

KEYS = cg.COUNTERS + lg.COUNTERS
_built = {}


def built(fx, tmp_path_factory):
    if fx.name not in _built:
        path = str(tmp_path_factory.mktemp("coop") / "c.paf")
        with open(path, "w") as f:
            f.write(cg.paf(fx))
        g = impg_amd.GpuImpg.from_paf(path, bidirectional=False)
        c = o.OracleIndex(paf_paths=[path], bidirectional=False, preparse=True)
        lay = cg.layout(fx)
        assert {g.seq_name(i): i for i in range(g.num_seqs())} == lay.ids == {c.seq_name(i): i for i in range(c.num_seqs())}
        assert g.num_entries() == sum(n for _, n, _, _ in lay.seg.values())
        g.set_option("walk_kernel", 0)  # (the per-query walk has a lookup of its own: every run here is the batch engine's)
        g.set_option("lookup_stats", 1)
        g.set_option("locality_min", 1)
        _built[fx.name] = (g, c, lay, {})
    return _built[fx.name]


def snapshot(g):
    return {k: g.counter(k) for k in KEYS + ("small_batches",)}


@pytest.mark.parametrize("name", list(cg.CASES))
def test_wave_paths(tmp_path_factory, name):
    case = cg.CASES[name]
    g, c, lay, cache = built(case.fixture, tmp_path_factory)
    try:
        for bi, batch in enumerate(case.batches):
            ranges = [(lay.n_seq + 5 if t == cg.BAD else lay.ids[t], s, e) for t, s, e in batch]
            for r in {r for r in ranges if r[0] >= lay.n_seq}:
                # a range on an id the index does not hold answers with its own row (impg.rs:1896), transitive or not; the oracle's
                # transitive tables have no entry for such an id and return nothing, so that answer is written out: its plain one
                own = c.query(*r)
                assert own.tolist() == [(r[0], r[1], r[2]) * 2]
                cache[(tuple(sorted(cg.M1.items())), r)] = (own, 0)
            for span in case.spans:
                g.set_option("lookup_coop_span", span)
                for kw in (dict(), cg.M1):
                    model = cg.counters_of(lay, batch, bool(kw), span)
                    for fuse in (1, 0):
                        g.set_option("fuse_final_level", fuse)
                        wide = {}
                        for coop in (1, 0):
                            g.set_option("lookup_coop", coop)
                            for form in FORMS:
                                tag = (name, bi, span, fuse, coop)
                                # Engine::run_small answers a plain query_batch of <= 64 ranges: no lookup order, no wave counted
                                small = form == "batch" and not kw and len(ranges) <= lg.SMALL_RANGES
                                want = dict(model) if coop and not small else dict(model, **dict.fromkeys(cg.COUNTERS, 0))
                                want["small_batches"] = int(small)
                                before = snapshot(g)
                                check_forms(g, c, ranges, kw, forms=(form,), cache=cache, tag=tag)
                                after = snapshot(g)
                                got = {k: after[k] - before[k] for k in before}
                                assert got == want, (tag, kw, form)
                                assert wide.setdefault(form, {k: got[k] for k in lg.COUNTERS}) == {k: got[k] for k in lg.COUNTERS}, (tag, kw, form)
    finally:
        g.set_option("lookup_coop_span", cg.CAP)
        g.set_option("lookup_coop", 1)
        g.set_option("fuse_final_level", 1)


def test_two_level_run_on_the_default_path(tmp_path):
    """The kernel serves a frontier that frontier_emit_kernel wrote (with its lookup-order keys beside the records): a two-level
    transitive run of a few hundred ranges, every option but the lookup order's threshold at its default."""
    text, _ = random_paf(31, 400, n_seq=6, seq_len=60000, self_aln=True)
    path = str(tmp_path / "w.paf")
    with open(path, "w") as f:
        f.write(text)
    g = impg_amd.GpuImpg.from_paf(path)
    c = o.OracleIndex(paf_paths=[path], preparse=True)
    rl = random_ranges(9, 300, c.num_seqs(), 60000, max_len=3000, min_len=200)
    kw = dict(transitive=True, max_depth=2, min_transitive_len=20)
    g.set_option("walk_kernel", 0)
    g.set_option("lookup_stats", 1)
    g.set_option("locality_min", 1)
    assert (g.counter("lookup_coop_waves"), g.counter("lookup_lane_waves_mixed"), g.counter("lookup_lane_waves_span")) == (0, 0, 0)
    cache = {}
    for coop in (1, 0):
        g.set_option("lookup_coop", coop)
        before = {k: g.counter(k) for k in cg.COUNTERS}
        check_forms(g, c, rl, kw, cache=cache, tag=("two levels", coop))
        rise = {k: g.counter(k) - before[k] for k in cg.COUNTERS}
        waves1 = (len(rl) + 63) // 64  # the first level's waves; the second level's frontier adds its own
        if coop:
            assert sum(rise.values()) > len(FORMS) * waves1 and rise["lookup_coop_waves"] > len(FORMS), rise
        else:
            assert not any(rise.values()), rise
    # lookup_coop_span: 4 .. LOOKUP_COOP_CAP
    for bad in (3, cg.CAP + 1, 0, -1):
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            g.set_option("lookup_coop_span", bad)
        assert e.value.code == impg_amd.IMPG_E_INVALID
    for ok in (4, cg.CAP):
        g.set_option("lookup_coop_span", ok)
    # without lookup_stats nothing is counted
    g.set_option("lookup_stats", 0)
    g.set_option("lookup_coop", 1)
    before = {k: g.counter(k) for k in cg.COUNTERS}
    g.query_batch_stats(rl, impg_amd.make_params(**kw))
    assert {k: g.counter(k) for k in cg.COUNTERS} == before
