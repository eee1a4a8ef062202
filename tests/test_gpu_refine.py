"""`impg refine` on the GPU: the support kernels against the host twin and the sequential restatement
(tests/refine_ref.py) on scripted and random rows, the search end to end on the device route and on the routes whose
rows cross PCIe, what is refused, the text and the command line."""
import os
import subprocess

import numpy as np
import pytest

import impg_amd
from impg_amd import _lib
from oracle import oracle as o
from tests import refine_ref as rr
from tests.test_refine_cpu import CASES, RUNS, SHAPE, random_batch, run_case
from tests.tp_gen import random_tp

pytestmark = pytest.mark.gpu


def test_scripted_rows_on_the_device():
    for c in CASES:
        want = ([w[0] for w in c["want"]], [w[1] for w in c["want"]])
        assert run_case(c, True) == want, c["name"]
        assert run_case(c, False) == want, c["name"]


def test_random_rows_on_the_device():
    """300 candidates of up to 200 rows, one candidate that is a single group of 5 000 rows (one lane's long run), one of
    70 000 rows (several workgroups in every sort, scan and compaction), a blacklist on half the sequences: the kernels
    against the twin everywhere, against the restatement on every tenth candidate and the two large ones."""
    rng = np.random.default_rng(23)
    n_seq = 20
    per, cands = random_batch(rng, 300, n_seq, 200)
    # one group: query 7 on target 3, a chain of touching pieces over the region with a few strays
    t, s, e = 3, 10_000, 60_000
    q0 = np.arange(5000) * 10
    chain = [(7, int(a), int(a) + 10, t, s - 5 + int(a), s + 5 + int(a)) for a in q0]
    chain += [(7, int(a), int(a) + 10, t, 90_000, 90_010) for a in q0[::500]]  # equal query intervals, elsewhere on the target
    order = rng.permutation(len(chain))
    per.append([(t, s, e, t, s, e)] + [chain[i] for i in order][:4999])
    cands.append((t, s, e))
    big, bc = random_batch(rng, 1, n_seq, 0)
    tb, sb, eb = bc[0]
    n = 70_000
    qa = rng.integers(0, 2000, n) * 25
    ta = sb + rng.integers(-40, 400, n) * 10
    rows = np.zeros(n, dtype=_lib.INTERVAL_DTYPE)
    rows["query_id"] = rng.integers(0, n_seq, n)
    rows["query_id"][rng.random(n) < 0.01] = rr.HOLE
    rows["q_first"], rows["q_last"] = qa, qa + rng.integers(0, 4, n) * 25
    rows["target_id"] = tb
    rows["t_first"], rows["t_last"] = ta, ta + rng.integers(0, 500, n) * 10
    per.append([tuple(int(v) for v in r) for r in rows.tolist()])
    cands.append((tb, sb, eb))
    per.append([])
    cands.append((0, 5, 10))
    ent = [int(v) for v in rng.integers(0, 6, n_seq)]
    ent[11] = rr.NO_KEY
    mx = [int(v) for v in rng.integers(0, 6, len(cands))]
    bl = {q: [(int(a), int(a) + int(w)) for a, w in zip(rng.integers(0, 50_000, 30), rng.integers(0, 300, 30))] for q in range(0, n_seq, 2)}
    a, off = rr.rows_array(per)
    thin = list(range(0, 300, 10)) + [300, 301, 302]
    for d, kw in ((0, dict()), (40, dict(entity_of=ent, max_entities=mx, blacklist=bl)), (-1, dict(blacklist=bl)), (1000, dict(entity_of=ent))):
        st_h, st_d = {}, {}
        host = impg_amd.support_rows(a, off, cands, n_seq, span_bp=300, merge_distance=d, on_host=True, stats=st_h, **kw)
        dev = impg_amd.support_rows(a, off, cands, n_seq, span_bp=300, merge_distance=d, on_host=False, stats=st_d, **kw)
        assert dev == host, (d, list(kw))
        assert st_d == st_h and st_h["longest_group"] >= 4999
        sub = rr.support_batch([per[i] for i in thin], [cands[i] for i in thin], 300, d, kw.get("entity_of"),
                               [mx[i] for i in thin] if "max_entities" in kw else None, kw.get("blacklist"))
        assert ([host[0][i] for i in thin], [host[1][i] for i in thin]) == sub, (d, list(kw))
    plain = impg_amd.support_rows(a, off, cands, n_seq, span_bp=300, merge_distance=40, on_host=True)
    assert plain[0][300] == 1 and plain[0][301] >= 1 and max(plain[0][:300]) >= 3  # the long chain covers; the inputs reach survivors
    counts = impg_amd.support_rows(a, off, cands, n_seq, span_bp=300, merge_distance=40, on_host=False, survivors=False)
    assert counts == plain[0]


def test_device_primitive_refuses_a_foreign_sequence_id():
    """The guard, not a crash: the row is rewritten before anything indexes with it, the call returns IMPG_E_INVALID after
    the kernels have run, and the next call answers."""
    good = [rr.SELF, rr.COVER1]
    for bad_id in (rr.N_SEQ, 0x7FFFFFFF, 0xFFFFFFFE):
        rows, off = rr.rows_array([good, [rr.SELF, (bad_id, 1, 2, 0, 1000, 2000)], good])
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            impg_amd.support_rows(rows, off, [rr.REGION] * 3, rr.N_SEQ, on_host=False, entity_of=[1] * rr.N_SEQ, blacklist={1: [(0, 1)]})
        assert e.value.code == impg_amd.IMPG_E_INVALID
    rows, off = rr.rows_array([good])
    assert impg_amd.support_rows(rows, off, [rr.REGION], rr.N_SEQ, on_host=False) == ([1], [[(1, 500, 1700)]])


# ---- the search ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("refine") / "refine.paf")
    impg_amd.synth_paf_text(path, rr.E2E_SEED, 2000, **SHAPE)
    c = o.OracleIndex(paf_paths=[path], preparse=True)
    return path, c, rr.e2e_loci(c), impg_amd.GpuImpg.from_paf(path), {}


def reference(world, level, kw, labels=None):
    """The restatement's records for a run, computed once and left unchanged."""
    path, c, loci, g, cache = world
    key = (level, tuple(sorted(kw.items())))
    if key not in cache:
        ref = rr.Refine(c, level=level, query_kw=kw, **rr.E2E_OPTS)
        cache[key] = (ref, ref.run(loci))
    return cache[key]


def keys(records):
    return [rr.record_key(r) for r in records]


def counters(g):
    return {k: g.counter(k) for k in ("refine_passes", "refine_candidates", "refine_parts", "refine_rows_to_host", "refine_longest_group")}


@pytest.mark.parametrize("level,kw", RUNS, ids=["sequence-plain", "sample-plain", "sequence-bfs", "sample-bfs"])
def test_search_on_the_device_route(world, level, kw):
    path, c, loci, g, _ = world
    ref, want = reference(world, level, kw)
    before = counters(g)
    got = g.refine(loci, impg_amd.make_params(**kw), level=level, **rr.E2E_OPTS)
    after = counters(g)
    assert keys(got.records) == keys(want)
    assert (got.text, got.support_text) == ref.text(want)
    assert after["refine_rows_to_host"] == before["refine_rows_to_host"]
    assert 1 <= got.passes <= 4 and after["refine_passes"] - before["refine_passes"] == got.passes
    assert after["refine_candidates"] - before["refine_candidates"] == got.candidates == ref.evaluations + len(loci)
    assert got.parts == got.passes + 1 and after["refine_longest_group"] >= 1
    # once more with every pass cut into parts
    g.set_option("chunk_ranges", 16)
    try:
        cut = g.refine(loci, impg_amd.make_params(**kw), level=level, **rr.E2E_OPTS)
    finally:
        g.set_option("chunk_ranges", 0)
    assert cut.parts >= got.parts + 4 and cut.passes == got.passes  # 40 loci in chunks of 16: pass 0 and the survivors' read are three parts each
    assert keys(cut.records) == keys(want)
    # and with the support on the host twin: the same records, the rows cross PCIe
    host = g.refine(loci, impg_amd.make_params(**kw), level=level, on_host=True, **rr.E2E_OPTS)
    assert keys(host.records) == keys(want)
    assert counters(g)["refine_rows_to_host"] > after["refine_rows_to_host"]


@pytest.mark.parametrize("fastga", [False, True], ids=["standard", "fastga"])
def test_search_on_a_tracepoint_index(fastga):
    d = random_tp(5 + fastga, 1500, n_seq=6, seq_len=120_000, fastga=fastga, max_segs=120)
    g = impg_amd.GpuImpg.from_tracepoints(d["records"], d["tracepoints"], d["seq_len"], query_deltas=d["query_deltas"], diffs=d["diffs"],
                                          fastga=d["fastga"], trace_spacing=d["trace_spacing"], max_complexity=d["max_complexity"])
    c = o.OracleIndex(tracepoints=d)
    rng = np.random.default_rng(3)
    loci = [(int(t), int(s), int(s) + 1500) for t, s in zip(rng.integers(0, 6, 30), rng.integers(0, 118_000, 30))] + [(2, 200, 1700), (4, 118_400, 119_900)]
    opts = dict(span_bp=200, max_extension=1.0, extension_step=500, merge_distance=3000)
    for kw in (dict(), dict(transitive=True, max_depth=2)):
        ref = rr.Refine(c, level="sequence", query_kw=kw, **opts)
        want = ref.run(loci)
        before = g.counter("refine_rows_to_host")
        got = g.refine(loci, impg_amd.make_params(**kw), **opts)
        assert keys(got.records) == keys(want), kw
        assert g.counter("refine_rows_to_host") == before and got.passes == 4
        assert any(r["support_count"] > 0 for r in want) and "clamped" in ref.seen


@pytest.mark.parametrize("level,kw", [("haplotype", dict(transitive=True, dfs=True, max_depth=2)), ("sample", dict(transitive=True, max_depth=2, multi_impg=True))],
                         ids=["dfs", "multi_impg"])
def test_search_on_the_routes_through_the_host(world, level, kw):
    path, c, loci, g, _ = world
    ref, want = reference(world, level, kw)
    before = counters(g)
    got = g.refine(loci, impg_amd.make_params(**kw), level=level, **rr.E2E_OPTS)
    assert keys(got.records) == keys(want)
    assert counters(g)["refine_rows_to_host"] > before["refine_rows_to_host"]
    assert {"left", "right", "rose", "stopped_at_max"} <= ref.seen


def test_subset_and_blacklist(world):
    path, c, loci, g, _ = world
    names = [c.seq_name(i) for i in range(c.num_seqs())]
    keep = np.array([0 if nm.startswith("g002#") else 1 for nm in names], dtype=np.uint8)
    assert 0 < keep.sum() < len(names)
    bl = {q: [(a, a + 4000) for a in range(0, 200_000, 40_000)] for q in range(0, len(names), 3)}
    for level, kw in (("sample", dict()), ("sample", dict(transitive=True, max_depth=2))):
        ref = rr.Refine(c, level=level, query_kw=kw, subset_keep=keep, blacklist=bl, **rr.E2E_OPTS)
        want = ref.run(loci)
        got = g.refine(loci, impg_amd.make_params(**kw), level=level, subset_keep=keep, blacklist=bl, **rr.E2E_OPTS)
        assert keys(got.records) == keys(want), kw
        plain, _ = reference(world, level, kw), None
        assert keys(want) != keys(plain[1])  # the filters change the answer


def test_refusals(world, tmp_path):
    path, c, loci, g, _ = world
    P = impg_amd.make_params
    cases = [(dict(params=P(store_cigar=True)), impg_amd.IMPG_E_INVALID), (dict(params=P(transitive=True, min_output_length=0)), impg_amd.IMPG_E_INVALID),
             (dict(loci=[(0, 500, 500)]), impg_amd.IMPG_E_INVALID), (dict(loci=[(0, 600, 500)]), impg_amd.IMPG_E_INVALID),
             (dict(loci=[(c.num_seqs(), 500, 2500)]), impg_amd.IMPG_E_INVALID), (dict(extension_step=0), impg_amd.IMPG_E_INVALID),
             (dict(extension_step=-5), impg_amd.IMPG_E_INVALID), (dict(span_bp=-1), impg_amd.IMPG_E_INVALID),
             (dict(max_extension=-1.0), impg_amd.IMPG_E_INVALID), (dict(loci=[(0, 300_000, 302_000)]), impg_amd.IMPG_E_INVALID)]
    t, s, e = loci[5]
    want = c.query(t, s, e).tolist()
    for kw, code in cases:
        kw = dict(kw)
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            g.refine(kw.pop("loci", loci[:3]), kw.pop("params", None), **kw)
        assert ei.value.code == code, kw
        assert g.query_batch([(t, s, e)], P())[0].tolist() == want
    multi = impg_amd.GpuImpg.from_paf(path, devices=[0, 0])
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        multi.refine(loci[:3])
    assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED
    assert multi.query_batch([(t, s, e)], P())[0].tolist() == want


def test_text_and_command_line(world, tmp_path):
    path, c, loci, g, _ = world
    kw = dict(transitive=True, max_depth=2)
    ref, want = reference(world, "sample", kw)
    labels = [".", "", "  ", "locus3"] + ["l%d" % i for i in range(4, len(loci))]
    labelled = [dict(r, label=labels[i]) for i, r in enumerate(want)]
    text, sup = ref.text(labelled)
    got = g.refine(loci, impg_amd.make_params(**kw), level="sample", names=labels, **rr.E2E_OPTS)
    assert (got.text, got.support_text) == (text, sup)
    assert text.count("\n") == len(loci) + 1 and sup.count("\n") == sum(len(r["survivors"]) for r in want) > 0
    names = ref.names
    assert text.splitlines()[1].split("\t")[3] == "%s:%d-%d" % (names[loci[0][0]], loci[0][1], loci[0][2])
    assert text.splitlines()[4].split("\t")[3] == "locus3"
    bed = tmp_path / "loci.bed"
    bed.write_text("".join("%s\t%d\t%d\t%s\n" % (names[t], s, e, labels[i]) for i, (t, s, e) in enumerate(loci)))
    out = tmp_path / "support.bed"
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "impg-gpu")
    r = subprocess.run([exe, "refine", "-a", path, "-b", str(bed), "-d", "5000", "--span-bp", "500", "--max-extension", "3000", "--extension-step", "500",
                        "--pansn-mode", "sample", "-x", "-m", "2", "--support-output", str(out)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == text
    assert out.read_text() == sup
    bad = subprocess.run([exe, "refine", "-a", path, "-b", str(bed), "-d", "0", "--extension-step", "0"], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"--extension-step must be > 0" in bad.stderr
