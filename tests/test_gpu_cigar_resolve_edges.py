"""The resolve kernels (impg_amd/csrc/cigar_resolve_device.hip) on the edges of their own geometry: the fixtures of
tests/eqx_edge_gen.py -- tests/test_eqx_edge_cpu.py asserts that each sits where it says -- at every tile size the pass
takes, against the model (tests/eqx_ref.py); the proof that the tile size asked for was the one used (the items that the
pass's timing line counts); and from_paf(path, resolve_matches=seqs), which always runs at the shipped tile, on multi-tile
ops against the oracle of the model's converted PAF.  Every comparison is exact equality."""
import numpy as np
import pytest

import impg_amd
from oracle import oracle as o
from tests import eqx_edge_gen as edge, eqx_gen as gen, eqx_ref as ref
from tests.test_eqx_cpu import same, sequences

pytestmark = pytest.mark.gpu

TILE_BASES = 1024  # cigar_resolve.hpp: what tile_bases = None (0 in the C call) means
TILES = (None, 64, 256, 1024, 2048, 4096)
CASES = [(name, t) for name in ("wide", "checked", "holes") for t in TILES] + [("chains", None), ("chains", 64)] + \
        [(name, t) for name in ("borders", "skew") for t in (2048, 4096)]
_SEQS = {}


def world(name):
    """the fixture (the old ones have no masks) and its sequences, uploaded once"""
    f = edge.fixture(name) if name in edge.ALL else gen.fixture(name)
    if name not in _SEQS:
        _SEQS[name] = sequences(f["store"])
    return f, _SEQS[name]


@pytest.mark.parametrize("name,tile", CASES)
def test_device_equals_model(name, tile):
    f, seqs = world(name)
    got = impg_amd.resolve_cigars(f["records"], f["ops"], f["names"], f["seq_len"], seqs, tile_bases=tile)
    same(got, f["model"], (name, tile))


@pytest.mark.parametrize("name", ("wide", "holes"))
def test_pool_addressed_in_any_order(name):
    f, seqs = world(name)
    rec, pool = edge.shuffled(f)
    for tile in (None, 4096):
        got = impg_amd.resolve_cigars(rec, pool, f["names"], f["seq_len"], seqs, tile_bases=tile)
        same(got, f["model"], (name, tile))


@pytest.mark.parametrize("name", edge.ALL)
def test_the_tile_size_asked_for_is_the_one_used(name, tmp_path, monkeypatch):
    """IMPG_RESOLVE_TIMING (read per call): every call appends a line whose items are the items that geometry() counts at
    that tile and at no other -- the answer itself does not depend on the tile, so nothing else could tell"""
    f, seqs = world(name)
    path = tmp_path / "timing.txt"
    monkeypatch.setenv("IMPG_RESOLVE_TIMING", str(path))
    tiles = (None, 64) if name == "chains" else TILES
    for tile in tiles:
        impg_amd.resolve_cigars(f["records"], f["ops"], f["names"], f["seq_len"], seqs, tile_bases=tile)
    lines = path.read_text().splitlines()
    assert len(lines) == len(tiles)
    items = []
    for tile, line in zip(tiles, lines):
        w = line.split()
        got = dict(zip(w[::2], w[1::2]))
        want = edge.geometry(f["records"], f["ops"], f["model"][2], f["masks"], tile or TILE_BASES, detail=False)["items"]
        print(name, tile, line)
        assert (int(got["items"]), int(got["ops_in"]), int(got["ops_out"])) == (want, len(f["ops"]), len(f["model"][1])), (name, tile)
        items.append(want)
    by_tile = dict(zip(tiles, items))
    others = [t for t in tiles if t != 1024]  # (None is 1024)
    assert len({by_tile[t] for t in others}) == len(others) >= 2  # every size cuts another number of items: the check above tells them apart


# ---- end to end at the shipped tile -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shipped(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("eqx_edges")
    f = edge.shipped()
    paf, fa, conv = str(tmp / "shipped.paf"), str(tmp / "shipped.fa"), str(tmp / "shipped.eqx.paf")
    for path, text in ((paf, f["paf"]), (fa, edge.fasta(f["store"])), (conv, ref.convert_paf(f["paf"], f["store"]))):
        with open(path, "w") as h:
            h.write(text)
    g = impg_amd.GpuImpg.from_paf(paf, resolve_matches=impg_amd.Sequences.from_fasta(fa))
    c = o.OracleIndex(paf_paths=[conv], preparse=True)
    assert [g.seq_name(i) for i in range(g.num_seqs())] == [c.seq_name(i) for i in range(c.num_seqs())] == f["names"]
    return dict(f=f, g=g, c=c, ranges=f["ranges"])


def test_shipped_rows_and_cigars_equal_the_oracle_of_the_converted_paf(shipped):
    g, c, rl = shipped["g"], shipped["c"], shipped["ranges"]
    rows = 0
    for kw in (dict(), dict(transitive=True, max_depth=3)):
        res = g.query_batch(rl, impg_amd.make_params(store_cigar=True, **kw))
        for i, (t, s, e) in enumerate(rl):
            want, cigars = c.query_cigar(t, s, e, **kw)
            assert res[i].tolist() == want.tolist(), (kw, i)
            assert [x.tolist() for x in res.cigars(i)] == [np.asarray(x).tolist() for x in cigars], (kw, i)
            rows += len(want)
    assert rows > 2 * len(rl)


def test_shipped_text_equals_the_oracle_of_the_converted_paf(shipped):
    g, c, rl = shipped["g"], shipped["c"], shipped["ranges"]
    rnames = ["r%d" % i for i in range(len(rl))]
    want = "".join(c.query_paf(c.seq_name(t), s, e, range_name=rn, merge_distance=0, fmt="paf") for (t, s, e), rn in zip(rl, rnames))
    assert g.query_batch_paf(rl, impg_amd.make_params(), merge_distance=0, range_names=rnames) == want
    assert want.count("\n") >= len(rl) and "X" in want


def test_shipped_report_and_counters(shipped):
    g, model = shipped["g"], shipped["f"]["model"]
    assert g.resolve_report() == model[3]
    assert g.resolve_flags.tolist() == model[2].tolist()
    assert g.counter("tokenized_device") == 1 and g.counter("build_device") == 1
