"""The resolve pass without a GPU: the model (tests/eqx_ref.py) on the hand-worked vectors, the host twin of the kernels
(impg_gpu_cigar_resolve, on_host = 1) against the model on every fixture of tests/eqx_gen.py, and the model's own identities."""
import numpy as np
import pytest

import impg_amd
from impg_amd import _lib
from tests import eqx_gen as gen, eqx_ref as ref


def sequences(store):
    names = list(store)
    return impg_amd.Sequences.from_arrays(names, [store[n] for n in names])


def same(got, want, what):
    """(records, ops, flags, report) of the library against the model's: everything, exactly"""
    rec, ops, flags, rep = got
    mrec, mops, mflags, mrep = want
    assert flags.tolist() == mflags.tolist(), what
    assert ops.tolist() == mops.tolist(), what
    assert rec.tobytes() == np.ascontiguousarray(mrec, dtype=_lib.RECORD_DTYPE).tobytes(), what
    assert rep == mrep, what


def test_hand_worked_vectors():
    for k, (t, q, strand, cg_in, cg_out) in enumerate(gen.VECTORS):
        rec = np.array([(0, 1, 0, len(q), 0, len(t), 0, 0, strand == "-")], dtype=ref.RECORD_DTYPE)
        ops = ref.pack(cg_in)
        rec[0]["cigar_len"] = len(ops)
        store = {"q": q.encode(), "t": t.encode()}
        out_rec, out, flags, rep = ref.resolve(rec, ops, ["q", "t"], [len(q), len(t)], store)
        assert ref.unpack(out) == cg_out and flags.tolist() == [0], (k, ref.unpack(out))
        got = impg_amd.resolve_cigars(rec, ops, ["q", "t"], [len(q), len(t)], sequences(store), on_host=True)
        assert ref.unpack(got[1]) == cg_out and got[2].tolist() == [0], (k, ref.unpack(got[1]))
        same(got, (out_rec, out, flags, rep), k)


@pytest.mark.parametrize("name", gen.ALL)
def test_host_twin_equals_model(name):
    f = gen.fixture(name)
    got = impg_amd.resolve_cigars(f["records"], f["ops"], f["names"], f["seq_len"], sequences(f["store"]), on_host=True)
    same(got, f["model"], name)


def test_pool_addressed_in_any_order():
    """the records' ops reversed record by record in the pool in: the pool out is the same"""
    f = gen.fixture("mixed")
    rec = f["records"].copy()
    parts, at = [], 0
    for i in reversed(range(len(rec))):
        a, n = int(rec[i]["cigar_off"]), int(rec[i]["cigar_len"])
        parts.append(f["ops"][a:a + n])
        rec[i]["cigar_off"] = at
        at += n
    got = impg_amd.resolve_cigars(rec, np.concatenate(parts), f["names"], f["seq_len"], sequences(f["store"]), on_host=True)
    same(got, f["model"], "shuffled")


@pytest.mark.parametrize("name", gen.ALL)
def test_model_identities(name):
    f = gen.fixture(name)
    out_rec, out, flags, rep = f["model"]
    assert rep["m_eq_bases"] + rep["m_x_bases"] == rep["m_bases"]
    assert rep["resolved"] + rep["absent"] + rep["inconsistent"] == int((f["records"]["cigar_len"] > 0).sum())
    runs = 0
    for r, o, fl in zip(f["records"], out_rec, flags):
        mine = f["ops"][int(r["cigar_off"]):int(r["cigar_off"]) + int(r["cigar_len"])]
        new = out[int(o["cigar_off"]):int(o["cigar_off"]) + int(o["cigar_len"])]
        if fl:
            assert new.tolist() == mine.tolist()
            continue
        assert ref.fuse_back(mine, new) == mine.tolist()  # fusing the runs back wherever the input had an M returns the input
        runs += len(new) - int(((mine >> 29) != 4).sum())
    assert rep["ops_out"] - rep["ops_in"] == runs - rep["m_ops"]
    if f["fx"] is not None:  # what the fixture planted is what the model counts
        planted = f["fx"].planted
        if name != "flags":
            assert (rep["m_x_bases"], rep["m_eq_bases"]) == (planted["m_x"], planted["m_eq"])
            assert (rep["bad_eq_bases"], rep["bad_x_bases"]) == (planted["bad_eq"], planted["bad_x"])


def test_fixtures_hold_what_they_promise():
    assert gen.fixture("flags")["model"][2].tolist() == [0, 1, 0, 2, 0, 2, 0, 2, 0]
    mixed = gen.fixture("mixed")
    assert mixed["model"][3]["bad_eq_bases"] == 12 and mixed["model"][3]["bad_x_bases"] == 6
    assert int((mixed["records"]["cigar_len"] == 0).sum()) == 1 and any(int(w) == 4 << 29 for w in mixed["ops"])
    b = gen.fixture("borders")
    q = {n: i for i, n in enumerate(b["names"])}
    for tile in gen.BORDER_TILES:
        mine = b["records"][b["records"]["query_id"] == q["Q%d" % tile]]
        assert mine["query_start"].min() == 0 and mine["query_end"].max() == b["seq_len"][q["Q%d" % tile]]
    assert set(b["records"]["target_start"].tolist()) == set(gen.BORDER_STARTS)
    assert any(len(s) != len(s.upper()) or s != s.upper() for s in gen.fixture("bytes")["store"].values())
    sk = gen.fixture("skew")["model"][3]
    assert sk["m_bases"] > 50000 and sk["records"] == 501


def test_converted_paf_round_trip():
    """the converted text parses to the model's pool, and converting it again changes nothing"""
    for name in ("mixed", "bytes", "flags"):
        f = gen.fixture(name)
        text = ref.convert_paf(f["paf"], f["store"])
        recs, ops, names, lens = ref.parse_paf(text)
        assert ops.tolist() == f["model"][1].tolist() and names == f["names"]
        assert ref.convert_paf(text, f["store"]) == text
        if name != "flags":
            assert "M" not in "".join(ln.split("cg:Z:")[1] for ln in text.splitlines() if "cg:Z:" in ln)


def test_refused_arguments_and_bindings():
    f = gen.fixture("vectors")
    seqs = sequences(f["store"])
    for bad in (1, 100, 4160):
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            impg_amd.resolve_cigars(f["records"], f["ops"], f["names"], f["seq_len"], seqs, on_host=True, tile_bases=bad)
        assert ei.value.code == impg_amd.IMPG_E_INVALID
    rec = f["records"].copy()
    rec[0]["cigar_off"] = len(f["ops"])
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        impg_amd.resolve_cigars(rec, f["ops"], f["names"], f["seq_len"], seqs, on_host=True)
    assert ei.value.code == impg_amd.IMPG_E_INVALID and "outside the op pool" in str(ei.value)
    assert {"resolve_" + k for k in ref.REPORT_FIELDS} <= set(impg_amd.counter_keys())
    assert tuple(_lib.RESOLVE_FIELDS) == ref.REPORT_FIELDS
    assert {"impg_gpu_cigar_resolve", "impg_gpu_selftest_cigar_resolve", "impg_gpu_index_create_from_paf_resolved"} <= {n for n, _, _ in _lib.SYMBOLS}
    assert not [k for k in impg_amd.option_keys() if "resolve" in k]  # (the pass adds no option)
    with pytest.raises(ValueError):
        impg_amd.GpuImpg.from_paf("x.paf", resolve_matches=seqs, ingest="device")
    with pytest.raises(ValueError):
        impg_amd.GpuImpg.from_paf("x.paf", resolve_matches=seqs, devices=[0])
