"""`impg refine` on the host twin (impg_gpu_support_rows / impg_gpu_refine_rows with on_host = 1; no GPU): the support
count against hand-worked answers and the sequential restatement of tests/refine_ref.py, the flank grid, and the whole
search over rows the CPU oracle hands out."""
import numpy as np
import pytest

import impg_amd
from impg_amd import _lib
from oracle import oracle as o
from tests import refine_ref as rr

CASES = rr.scripted_cases()


def run_case(c, on_host):
    rows, off = rr.rows_array(c["rows"])
    return impg_amd.support_rows(rows, off, c["cands"], rr.N_SEQ, span_bp=c["span_bp"], merge_distance=c["d"], entity_of=c["entity_of"],
                                 max_entities=c["max_entities"], blacklist=c["blacklist"], on_host=on_host)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_scripted_known_answers(c):
    want_count, want_surv = [w[0] for w in c["want"]], [w[1] for w in c["want"]]
    # the restatement gives the hand-worked answer ...
    assert rr.support_batch(c["rows"], c["cands"], c["span_bp"], c["d"], c["entity_of"], c["max_entities"], c["blacklist"]) == (want_count, want_surv)
    # ... and so does the twin
    assert run_case(c, True) == (want_count, want_surv)


def test_scripted_cases_cover_the_list():
    names = {c["name"] for c in CASES}
    assert {"one_row", "query_adjacent", "target_adjacent", "overlap_no_merge", "tie_xy", "tie_yx", "reverse", "hole_and_own_target", "no_rows",
            "no_merge", "span_beyond_region", "negative_span", "cover_miss_start", "cover_miss_end", "cover_miss_left_threshold",
            "cover_miss_right_threshold", "bl_end_at_lo", "bl_start_at_hi", "bl_start_behind_hi", "bl_overlapping_hit", "two_of_one_entity",
            "no_key", "clamp", "batch"} <= names
    tie = {c["name"]: c for c in CASES}
    assert sorted(tie["tie_xy"]["rows"][0]) == sorted(tie["tie_yx"]["rows"][0]) and tie["tie_xy"]["want"] != tie["tie_yx"]["want"]


def random_batch(rng, n_cand, n_seq, max_rows, span=300):
    """Candidates on random targets with rows that cover, nearly cover, touch each other and repeat their query interval."""
    per, cands = [], []
    for _ in range(n_cand):
        t = int(rng.integers(n_seq))
        s = int(rng.integers(0, 5000))
        e = s + int(rng.integers(1, 4000))
        rows = [(t, s, e, t, s, e)] if rng.random() < 0.9 else []
        for _ in range(int(rng.integers(0, max_rows + 1))):
            kind = rng.random()
            q = int(rng.integers(n_seq)) if kind > 0.03 else rr.HOLE
            qa = int(rng.integers(0, 60)) * 50  # a coarse grid: equal and touching intervals are common
            qb = qa + int(rng.integers(0, 8)) * 50
            if kind < 0.5:  # around the region
                ta, tb = s - int(rng.integers(-2, 3)), e + int(rng.integers(-2, 3))
            else:  # a piece of it, on the grid
                ta = s + int(rng.integers(-4, 40)) * 100
                tb = ta + int(rng.integers(0, 40)) * 100
            if rng.random() < 0.3:
                qa, qb = qb, qa
            if rng.random() < 0.1:
                ta, tb = tb, ta
            rows.append((q, qa, qb, t, ta, tb))
        per.append(rows)
        cands.append((t, s, e))
    return per, cands


@pytest.mark.parametrize("d", [-1, 0, 100, 1000])
def test_random_rows_against_the_restatement(d):
    rng = np.random.default_rng(11 + d)
    per, cands = random_batch(rng, 120, 12, 40)
    ent = [int(v) for v in rng.integers(0, 5, 12)]
    ent[3] = rr.NO_KEY
    mx = [int(v) for v in rng.integers(0, 4, len(cands))]
    bl = {s: [(int(a), int(a) + int(w)) for a, w in zip(rng.integers(0, 3000, 4), rng.integers(0, 400, 4))] for s in range(0, 12, 2)}
    rows, off = rr.rows_array(per)
    for kw in (dict(), dict(entity_of=ent), dict(entity_of=ent, max_entities=mx), dict(blacklist=bl), dict(entity_of=ent, max_entities=mx, blacklist=bl)):
        want = rr.support_batch(per, cands, 300, d, kw.get("entity_of"), kw.get("max_entities"), kw.get("blacklist"))
        got = impg_amd.support_rows(rows, off, cands, 12, span_bp=300, merge_distance=d, on_host=True, **kw)
        assert got == want, kw.keys()
    counts = rr.support_batch(per, cands, 300, d)[0]
    assert max(counts) >= 3 and min(counts) == 0  # the inputs reach both ends


def test_primitive_refusals():
    rows, off = rr.rows_array([[rr.SELF, (rr.N_SEQ, 1, 2, 0, 1000, 2000)]])
    for bad in (dict(rows=rows, off=off, bl=None), dict(rows=rows[:1], off=off[:1].tolist() + [1], bl={1: [(5, 4)]})):
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            impg_amd.support_rows(bad["rows"], bad["off"], [rr.REGION], rr.N_SEQ, blacklist=bad["bl"], on_host=True)
        assert e.value.code == impg_amd.IMPG_E_INVALID
    with pytest.raises(impg_amd.ImpgGpuError) as e:  # offsets that descend
        impg_amd.support_rows(rows, [0, 2, 1], [rr.REGION, rr.REGION], rr.N_SEQ, on_host=True)
    assert e.value.code == impg_amd.IMPG_E_INVALID


def test_entity_ids():
    names = ["A#1#chr1", "A#1#chr2", "A#2#chr1", "B#1#chr1", "plain", "C#1", "A"]
    s, n = impg_amd.entity_ids(names, "sample")
    assert n == 3 and s.tolist() == [0, 0, 0, 1, rr.NO_KEY, 2, rr.NO_KEY]
    h, n = impg_amd.entity_ids(names, "haplotype")
    assert n == 4 and h.tolist() == [0, 0, 1, 2, rr.NO_KEY, 3, rr.NO_KEY]
    for lv, got in (("sample", s), ("haplotype", h)):  # the restatement's keys group the names the same way
        keys = [rr.pansn_key(nm, lv) for nm in names]
        assert [k is None for k in keys] == [v == rr.NO_KEY for v in got.tolist()]
        assert len({(k, v) for k, v in zip(keys, got.tolist())}) == len(set(keys))
    assert impg_amd.entity_ids(["x|y|z", "x|w|z"], "haplotype", "|")[0].tolist() == [0, 1]


# 17: build_flanks(max_extension_bp, step), and both readings of --max-extension for a locus of 2000 bp
FLANKS = [((0, 500), [0]), ((3000, 1000), [0, 1000, 2000, 3000]), ((2500, 1000), [0, 1000, 2000, 2500]), ((300, 1000), [0, 300]),
          ((1, 1), [0, 1]), ((1000, 1000), [0, 1000])]
READINGS = [(0.0, 0), (0.5, 1000), (1.0, 2000), (1.5, 2), (2500, 2500), (0.0004, 1), (2500.2, 2501)]


def test_build_flanks_and_max_extension():
    for (mx, step), want in FLANKS:
        assert rr.build_flanks(mx, step) == want, (mx, step)
    for me, want in READINGS:
        assert rr.max_extension_bp(me, 2000) == want, me


def test_flank_grid_of_the_search():
    """The library's grid, seen through the regions it asks a row source for: a locus of 2000 bp in the middle of a long
    sequence, no rows at all (so no pass stops early): pass 1 asks (l, 0) for l > 0, passes 2 and 3 every flank."""
    for me, step in [(0.0, 500), (3000, 1000), (2500, 1000), (300, 1000), (0.5, 1000), (1.0, 700), (1.5, 1), (2500.2, 5000)]:
        flanks = rr.build_flanks(rr.max_extension_bp(me, 2000), step)
        asked = []

        def query(regions):
            asked.append(list(regions))
            return [np.zeros(0, dtype=_lib.INTERVAL_DTYPE) for _ in regions]

        res = impg_amd.refine_rows(query, [100000], [(0, 50000, 52000)], max_extension=me, extension_step=step)
        assert asked[0] == [(0, 50000, 52000)]
        assert asked[1] == [(0, 50000 - l, 52000) for l in flanks if l > 0] or (flanks == [0] and asked[1] == [(0, 50000, 52000)])
        if flanks != [0]:
            assert asked[2] == [(0, 50000, 52000 + r) for r in flanks] and asked[3] == [(0, 50000 - l, 52000) for l in flanks]
        assert res[0]["support_count"] == 0 and res[0]["left_extension"] == 0 and res[0]["right_extension"] == 0
        assert res.passes == len(asked) - 1  # the last call reads the winners' survivors


def test_search_refusals():
    none = lambda regions: [np.zeros(0, dtype=_lib.INTERVAL_DTYPE) for _ in regions]
    for kw, loci in ((dict(extension_step=0), [(0, 10, 20)]), (dict(span_bp=-1), [(0, 10, 20)]), (dict(max_extension=-0.5), [(0, 10, 20)]),
                     (dict(), [(0, 20, 20)]), (dict(), [(0, 30, 20)]), (dict(), [(3, 10, 20)]), (dict(), [(0, 2000, 2100)])):
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            impg_amd.refine_rows(none, [1000], loci, **kw)
        assert e.value.code == impg_amd.IMPG_E_INVALID, (kw, loci)


# ---- end to end: the search over the oracle's rows ------------------------------------------------------------------------
SHAPE = dict(n_seq=20, seq_len=200000, target_span=10000, n_blocks=100)
RUNS = [("sequence", dict()), ("sample", dict()), ("sequence", dict(transitive=True, max_depth=2)), ("sample", dict(transitive=True, max_depth=2))]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("refine") / "refine.paf")
    impg_amd.synth_paf_text(path, rr.E2E_SEED, 2000, **SHAPE)
    c = o.OracleIndex(paf_paths=[path], preparse=True)
    loci = rr.e2e_loci(c)
    return path, c, loci


def oracle_rows(c, kw):
    def query(regions):
        return [c.query(t, s, e, **kw) for t, s, e in regions]
    return query


@pytest.mark.parametrize("level,kw", RUNS, ids=["sequence-plain", "sample-plain", "sequence-bfs", "sample-bfs"])
def test_search_end_to_end_on_host(world, level, kw):
    path, c, loci = world
    ref = rr.Refine(c, level=level, query_kw=kw, **rr.E2E_OPTS)
    want = ref.run(loci)
    names = ref.names
    lens = [c.seq_len(i) for i in range(len(names))]
    ent = None if level == "sequence" else impg_amd.entity_ids(names, level)[0]
    mx = None if level == "sequence" else [ref.compute_max_entities(t) for t, _, _ in loci]
    got = impg_amd.refine_rows(oracle_rows(c, kw), lens, loci, entity_of=ent, max_entities=mx, on_host=True, names=names, **rr.E2E_OPTS)
    assert [rr.record_key(r) for r in got.records] == [rr.record_key(r) for r in want]
    assert (got.text, got.support_text) == ref.text(want)
    assert got.passes <= 4
    # the inputs exercise the search (on the restatement's own output)
    need = {"left", "right", "rose", "clamped"} | ({"stopped_at_max"} if level != "sequence" else set())
    assert need <= ref.seen, need - ref.seen
