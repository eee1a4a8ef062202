"""The resolve pass on the device (impg_amd/csrc/cigar_resolve_device.hip): kernels == host twin == model
(tests/eqx_ref.py) on every fixture of tests/eqx_gen.py, then end to end -- from_paf(path, resolve_matches=seqs) against the
oracle built from the model's converted PAF.  Every comparison is exact equality; every case is small."""
import os
import subprocess

import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import eqx_gen as gen, eqx_ref as ref
from tests.test_eqx_cpu import same, sequences

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(impg_amd.__file__), "impg-gpu")
E2E = ("mixed", "bytes", "random")


@pytest.mark.parametrize("name", gen.ALL)
def test_device_equals_host_twin_equals_model(name):
    f = gen.fixture(name)
    seqs = sequences(f["store"])
    host = impg_amd.resolve_cigars(f["records"], f["ops"], f["names"], f["seq_len"], seqs, on_host=True)
    same(host, f["model"], name)
    for tile in (None, 64, 256) if name in ("borders", "skew", "mixed") else (None, 64):
        got = impg_amd.resolve_cigars(f["records"], f["ops"], f["names"], f["seq_len"], seqs, tile_bases=tile)
        same(got, f["model"], (name, tile))


def test_pool_addressed_in_any_order():
    f = gen.fixture("random")
    rec = f["records"].copy()
    parts, at = [], 0
    for i in reversed(range(len(rec))):
        a, n = int(rec[i]["cigar_off"]), int(rec[i]["cigar_len"])
        parts.append(f["ops"][a:a + n])
        rec[i]["cigar_off"] = at
        at += n
    got = impg_amd.resolve_cigars(rec, np.concatenate(parts), f["names"], f["seq_len"], sequences(f["store"]))
    same(got, f["model"], "shuffled")


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    """per end-to-end fixture: the resolved index, the unresolved one, the oracle of the converted PAF, 40 ranges, the paths"""
    tmp = tmp_path_factory.mktemp("eqx")
    out = {}
    for name in E2E:
        f = gen.fixture(name)
        if "cg:Z:" not in f["paf"].splitlines()[17]:  # the reference refuses a file with a line without cg:Z (the pass's own tests keep it)
            text = "".join(ln + "\n" for ln in f["paf"].splitlines() if "cg:Z:" in ln)
            recs, ops, names, lens = ref.parse_paf(text)
            f = dict(f, paf=text, records=recs, ops=ops, names=names, seq_len=lens, model=ref.resolve(recs, ops, names, lens, f["store"]))
        paf, fa, conv = str(tmp / (name + ".paf")), str(tmp / (name + ".fa")), str(tmp / (name + ".eqx.paf"))
        with open(paf, "w") as h:
            h.write(f["paf"])
        with open(fa, "w") as h:
            h.write(f["fx"].fasta())
        with open(conv, "w") as h:
            h.write(ref.convert_paf(f["paf"], f["store"]))
        seqs = impg_amd.Sequences.from_fasta(fa)
        g = impg_amd.GpuImpg.from_paf(paf, resolve_matches=seqs)
        plain = impg_amd.GpuImpg.from_paf(paf)
        c = o.OracleIndex(paf_paths=[conv], preparse=True)
        assert [g.seq_name(i) for i in range(g.num_seqs())] == [c.seq_name(i) for i in range(c.num_seqs())] == f["names"]
        rng, rl = np.random.default_rng(7), []
        for k in range(40):  # ranges that begin inside a record's target interval
            r = f["records"][(k * 7) % len(f["records"])]
            a = int(r["target_start"]) + int(rng.integers(0, max((int(r["target_end"]) - int(r["target_start"])) // 2, 1)))
            rl.append((int(r["target_id"]), a, min(a + int(rng.integers(150, 1500)), int(f["seq_len"][r["target_id"]]))))
        out[name] = dict(f=f, g=g, plain=plain, c=c, ranges=rl, paf=paf, fa=fa, conv=conv)
    return out


@pytest.mark.parametrize("name", E2E)
def test_rows_and_cigars_equal_the_oracle_of_the_converted_paf(worlds, name):
    w = worlds[name]
    g, c, rl = w["g"], w["c"], w["ranges"]
    assert len(rl) >= 32
    rows = 0
    for kw in (dict(), dict(transitive=True, max_depth=3)):
        res = g.query_batch(rl, impg_amd.make_params(store_cigar=True, **kw))
        for i, (t, s, e) in enumerate(rl):
            want, cigars = c.query_cigar(t, s, e, **kw)
            assert res[i].tolist() == want.tolist(), (name, kw, i)
            assert [x.tolist() for x in res.cigars(i)] == [np.asarray(x).tolist() for x in cigars], (name, kw, i)
            rows += len(want)
    assert rows > 2 * len(rl)


@pytest.mark.parametrize("name", E2E)
def test_text_equals_the_oracle_of_the_converted_paf(worlds, name):
    w = worlds[name]
    g, c, rl = w["g"], w["c"], w["ranges"]
    rnames = ["r%d" % i for i in range(len(rl))]
    for fmt, call in (("paf", g.query_batch_paf), ("bedpe", g.query_batch_bedpe)):
        want = "".join(c.query_paf(c.seq_name(t), s, e, range_name=rn, merge_distance=0, fmt=fmt) for (t, s, e), rn in zip(rl, rnames))
        assert call(rl, impg_amd.make_params(), merge_distance=0, range_names=rnames) == want, (name, fmt)
        assert want.count("\n") >= len(rl)


def test_identity_filter_sees_the_mismatches(worlds):
    """0.85 lies between the records planted at 1 % and at 30 %: the resolved index answers as the oracle of the converted
    PAF does and drops rows that the unresolved index of the same file keeps -- what the pass is for"""
    w = worlds["random"]
    g, plain, c, rl = w["g"], w["plain"], w["c"], w["ranges"]
    p = impg_amd.make_params(min_identity=0.85)
    res, unresolved = g.query_batch(rl, p), plain.query_batch(rl, p)
    gone = 0
    for i, (t, s, e) in enumerate(rl):
        assert res[i].tolist() == c.query(t, s, e, min_identity=0.85).tolist(), i
        kept = {tuple(r) for r in res[i].tolist()}
        gone += sum(tuple(r) not in kept for r in unresolved[i].tolist())
    assert gone >= 1
    names = [g.seq_name(int(r["query_id"])) for i in range(len(rl)) for r in res[i]]
    assert [n for n in names if n.startswith("Q1_")]


@pytest.mark.parametrize("name", E2E)
def test_report_and_counters(worlds, name):
    w = worlds[name]
    model = w["f"]["model"]
    assert w["g"].resolve_report() == model[3]
    assert {k: w["g"].counter("resolve_" + k) for k in ref.REPORT_FIELDS} == model[3]
    assert w["g"].resolve_flags.tolist() == model[2].tolist()
    assert all(v == 0 for v in w["plain"].resolve_report().values())
    assert w["g"].counter("tokenized_device") == 1 and w["g"].counter("build_device") == 1


def test_flags_do_not_fail_the_build(tmp_path):
    f = gen.fixture("flags")
    fx = f["fx"]
    text = "".join(ln + "\n" for i, ln in enumerate(f["paf"].splitlines()) if i != 3)  # (without the interval past its sequence's end: the pass's own tests keep it)
    store = f["store"]
    paf, fa = str(tmp_path / "f.paf"), str(tmp_path / "f.fa")
    with open(paf, "w") as h:
        h.write(text)
    with open(fa, "w") as h:
        h.write(fx.fasta())
    recs, ops, names, lens = ref.parse_paf(text)
    model = ref.resolve(recs, ops, names, lens, store)
    g = impg_amd.GpuImpg.from_paf(paf, resolve_matches=impg_amd.Sequences.from_fasta(fa), bidirectional=False)
    assert g.resolve_report() == model[3] and g.resolve_flags.tolist() == model[2].tolist() == [0, 1, 0, 0, 2, 0, 2, 0]
    c = o.OracleIndex(paf_text=ref.convert_paf(text, store), bidirectional=False)
    t = g.seq_id("T")
    res = g.query_batch([(t, 0, 5000)], impg_amd.make_params(store_cigar=True))
    want, cigars = c.query_cigar(t, 0, 5000)
    assert res[0].tolist() == want.tolist() and [x.tolist() for x in res.cigars(0)] == [np.asarray(x).tolist() for x in cigars]


def test_refusals(worlds):
    w = worlds["mixed"]
    seqs = impg_amd.Sequences.from_fasta(w["fa"])
    for kw in (dict(ingest="device"), dict(devices=[0])):
        with pytest.raises(ValueError):
            impg_amd.GpuImpg.from_paf(w["paf"], resolve_matches=seqs, **kw)
    bed = os.path.join(os.path.dirname(w["paf"]), "one.bed")
    with open(bed, "w") as h:
        h.write("%s\t%d\t%d\tx\n" % ((w["g"].seq_name(w["ranges"][0][0]),) + tuple(w["ranges"][0][1:])))
    base = [CLI, "query", "-b", bed, "-d", "0", "-o", "paf", "--resolve-matches"]
    cases = [(["-a", w["paf"], "-i", os.path.join(os.path.dirname(w["paf"]), "saved.idx"), "--sequence-files", w["fa"]], "-i"),
             (["-a", w["paf"], "--sequence-files", w["fa"], "--alignment-ingest", "device"], "--alignment-ingest device"),
             (["-a", w["paf"], "--sequence-files", w["fa"], "--sequence-ingest", "device"], "--sequence-ingest device"),
             (["-a", w["paf"]], "--sequence-files")]
    for extra, words in cases:
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and "--resolve-matches" in r.stderr and words in r.stderr and r.stdout == "", (extra, r.stderr)


def test_cli_prints_the_oracles_text(worlds):
    w = worlds["random"]
    g, c, rl = w["g"], w["c"], w["ranges"]
    rnames = ["r%d" % i for i in range(len(rl))]
    bed = os.path.join(os.path.dirname(w["paf"]), "q.bed")
    with open(bed, "w") as h:
        for (t, s, e), rn in zip(rl, rnames):
            h.write("%s\t%d\t%d\t%s\n" % (g.seq_name(t), s, e, rn))
    want = "".join(c.query_paf(c.seq_name(t), s, e, range_name=rn, merge_distance=0, fmt="paf") for (t, s, e), rn in zip(rl, rnames))
    r = subprocess.run([CLI, "query", "-a", w["paf"], "-b", bed, "-d", "0", "-o", "paf", "--resolve-matches", "--sequence-files", w["fa"], "-v", "1"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    rep = w["f"]["model"][3]
    line = [ln for ln in r.stderr.splitlines() if "resolve-matches:" in ln]
    assert len(line) == 1 and "M ops %d bases %d = %d X %d" % (rep["m_ops"], rep["m_bases"], rep["m_eq_bases"], rep["m_x_bases"]) in line[0]
    for cmd in (["partition", "-w", "5000", "-d", "100"], ["refine", "-b", bed, "-d", "0"]):
        r = subprocess.run([CLI] + cmd + ["-a", w["paf"], "--resolve-matches", "--sequence-files", w["fa"], "-v", "1"] +
                           (["--output-folder", os.path.dirname(w["paf"])] if cmd[0] == "partition" else []), capture_output=True, text=True)
        assert r.returncode == 0 and "resolve-matches: records %d resolved %d" % (rep["records"], rep["resolved"]) in r.stderr, (cmd, r.stderr)
