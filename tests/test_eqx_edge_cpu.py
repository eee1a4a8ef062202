"""The fixtures of tests/eqx_edge_gen.py without a GPU: the host twin equals the model on each, and each sits on the edge it
names -- asserted with geometry(), which restates how the kernels cut their work, on the masks the fixtures were built from.
These are properties of the fixtures, not of the library: they are what makes tests/test_gpu_cigar_resolve_edges.py mean
something."""
import numpy as np
import pytest

import impg_amd
from tests import eqx_edge_gen as edge, eqx_gen as gen, eqx_ref as ref
from tests.test_eqx_cpu import same, sequences


def geometry(f, tile, **kw):
    return edge.geometry(f["records"], f["ops"], f["model"][2], f["masks"], tile, **kw)


@pytest.mark.parametrize("name", edge.ALL)
def test_host_twin_equals_model(name):
    f = edge.fixture(name)
    got = impg_amd.resolve_cigars(f["records"], f["ops"], f["names"], f["seq_len"], sequences(f["store"]), on_host=True)
    same(got, f["model"], name)


@pytest.mark.parametrize("name", ("wide", "holes"))
def test_pool_addressed_in_any_order(name):
    f = edge.fixture(name)
    rec, pool = edge.shuffled(f)
    assert pool.tolist() != f["ops"].tolist()
    got = impg_amd.resolve_cigars(rec, pool, f["names"], f["seq_len"], sequences(f["store"]), on_host=True)
    same(got, f["model"], name)


@pytest.mark.parametrize("name", edge.ALL)
def test_masks_are_what_the_model_sees(name):
    """the model's runs of every M op of a resolved record are the runs of the mask it was built from, and its counts are
    the planted ones: geometry() speaks about the bases that the kernels read"""
    f = edge.fixture(name)
    out_rec, out, flags, rep = f["model"]
    for i, (r, o) in enumerate(zip(f["records"], out_rec)):
        if flags[i] or not r["cigar_len"]:
            continue
        want = []
        for k in range(int(r["cigar_len"])):
            w = int(f["ops"][int(r["cigar_off"]) + k])
            if w >> 29 == 4:
                want.extend(c << 29 | n for c, n in ref.runs(f["masks"][(i, k)]))
            else:
                want.append(w)
        assert out[int(o["cigar_off"]):int(o["cigar_off"]) + int(o["cigar_len"])].tolist() == want, (name, i)
    if name != "holes":  # (whose flagged record plants bases that nobody counts)
        planted = f["fx"].planted
        assert (rep["m_x_bases"], rep["m_eq_bases"]) == (planted["m_x"], planted["m_eq"])
        assert (rep["bad_eq_bases"], rep["bad_x_bases"]) == (planted["bad_eq"], planted["bad_x"])


def test_geometry_on_a_hand_worked_case():
    """10M 3I 130M at tile 64: positions 0..9 | 0..129 with mismatches at 63, 64 and 129; one 200= and a flagged record"""
    d = gen.at(130, 63, 64, 129)
    rec = np.array([(0, 1, 0, 143, 0, 140, 0, 3, 0), (0, 1, 0, 200, 0, 200, 3, 1, 0), (0, 1, 0, 500, 0, 500, 4, 1, 0), (0, 1, 0, 0, 0, 0, 5, 0, 0)],
                   dtype=ref.RECORD_DTYPE)
    ops = np.array([4 << 29 | 10, 2 << 29 | 3, 4 << 29 | 130, 200, 4 << 29 | 500], dtype=np.uint32)
    g = edge.geometry(rec, ops, [0, 0, 2, 0], {(0, 0): gen.at(10), (0, 2): d}, 64)
    assert g["items"] == 1 + 1 + 3 + 4 + 1
    t = [(x["record"], x["op"], x["code"], x["k"], x["bases"], x["chunks"], x["starts"]) for x in g["tiles"]]
    assert t == [(0, 0, 4, 0, 10, 1, [0]), (0, 2, 4, 0, 64, 1, [0, 63]), (0, 2, 4, 1, 64, 1, [1]), (0, 2, 4, 2, 2, 1, [1]),
                 (1, 0, 0, 0, 64, 1, None), (1, 0, 0, 1, 64, 1, None), (1, 0, 0, 2, 64, 1, None), (1, 0, 0, 3, 8, 1, None)]
    assert g["chains"] == []
    g = edge.geometry(rec, ops, [0, 0, 0, 0], {(0, 0): gen.at(10), (0, 2): d, (2, 0): gen.at(500, 70, 71, 72, 400)}, 64)
    assert g["items"] == 1 + 1 + 3 + 4 + 8 and g["chains"] == [4, 1]  # starts at 0, 70, 73, 400, 401: tiles 2..5 and 7 have none
    assert [x["chunks"] for x in edge.geometry(rec, ops, [0, 0, 0, 0], {(0, 0): gen.at(10), (0, 2): d, (2, 0): gen.at(500)}, 256)["tiles"]] == [1, 3, 4, 4, 4]


@pytest.mark.parametrize("T", edge.WIDE_TILES)
def test_wide_sits_on_its_edges(T):
    f = edge.fixture("wide")
    fx, recs = f["fx"], f["records"]
    assert len(recs) <= 700 and not f["model"][2].any()
    q = f["names"].index("Q%d" % T)
    mine = [i for i in range(len(recs)) if recs[i]["query_id"] == q]
    assert [i for i, c in fx.cases.items() if c[0] == T] == mine
    assert recs[mine]["query_start"].min() == 0 and recs[mine]["query_end"].max() == f["seq_len"][q]
    assert set(recs["target_start"].tolist()) == set(gen.BORDER_STARTS)
    for L in edge.wide_lengths(T):  # every length on both strands, and the last tiles of 1 and of 63 bases
        assert {c[3] for c in fx.cases.values() if c[:2] == (T, L)} == {"+", "-"}
    assert {L % T for L in edge.wide_lengths(T)} >= {T - 1, 0, 1, 7, 63}
    tiles = [t for t in geometry(f, T)["tiles"] if t["record"] in set(mine)]
    nch = T // 64
    strands = lambda ts: {fx.cases[t["record"]][3] for t in ts}
    both = {"+", "-"}
    # the loop of four chunks: chunk counts that it does not divide, and its whole trips
    assert {t["chunks"] for t in tiles} >= {1, 7, nch} and strands([t for t in tiles if t["chunks"] == 7]) == both
    assert strands([t for t in tiles if t["chunks"] == nch and t["bases"] == T and t["k"] > 0]) == both
    assert any(t["chunks"] == nch and t["bases"] == T - 1 for t in tiles)  # the widest tile with a partial last chunk
    # a multi-tile M on the '+' strand whose tiles behind the first have starts of their own
    assert "+" in strands([t for t in tiles if t["k"] > 0 and t["starts"]])
    # a tile whose only start lies in its last chunk, in a first tile never (position 0 starts a run)
    only_last = [t for t in tiles if len(t["starts"]) == 1 and t["starts"][0] // 64 == t["chunks"] - 1 and t["chunks"] == nch]
    assert strands(only_last) == both
    if T == 4096:  # lane 63 holds a chunk
        assert nch == 64 and strands([t for t in tiles if t["bases"] == T and t["starts"] and t["starts"][-1] // 64 == 63]) == both
        assert strands([t for t in tiles if len(t["starts"]) == 4096]) == both  # every position a start
    # a start whose run ends at a start of the tile's last chunk with no start between them: `nxt` from chunk 0 across the wave
    far = [t for t in tiles if t["chunks"] == nch and any(a // 64 == 0 and b // 64 == nch - 1 for a, b in zip(t["starts"], t["starts"][1:]))]
    assert strands(far) == both and {t["k"] for t in far} >= {0, 1}
    # starts on both sides of every chunk border named, in tiles of T / 64 chunks and of 7
    for n, cs in ((nch, edge.WIDE_CHUNKS + (nch - 1,)), (7, edge.WIDE_CHUNKS + (6,))):
        for c in cs:
            at_border = [t for t in tiles if t["chunks"] == n and t["starts"]]
            for want in ({64 * c - 1}, {64 * c}, {64 * c + 1}):  # (a mismatch at p starts runs at p and p + 1)
                assert strands([t for t in at_border if want <= set(t["starts"]) and len(t["starts"]) <= 4]) == both, (n, c, want)
    # ... and on both sides of the tile's border
    for want in ([T - 1], [0], [1], [0, 1]):
        assert strands([t for t in tiles if t["starts"][-len(want):] == want and t["k"] == (want[0] != T - 1)]) == both, want
    # a run crossing each border named: the tile's, and each chunk's
    def classes_over(L, b):
        """(class, strand) of the runs with positions on both sides of border b, over the records of L bases"""
        d = {i: f["masks"][(i, 0)] for i, case in fx.cases.items() if case[:2] == (T, L)}
        return {(bool(m[b]), fx.cases[i][3]) for i, m in d.items() if m[b - 1] == m[b]}
    every = {(x, s) for x in (False, True) for s in "+-"}  # an '=' run and an 'X' run, on both strands
    for L in (T + 1, 2 * T + 1, 3 * T + 7):
        assert classes_over(L, T) == every, L
    for c in edge.WIDE_CHUNKS + (nch - 1,):
        for L, b in ((T, 64 * c), (3 * T + 7, T + 64 * c)):
            assert classes_over(L, b) == every, (c, L)
    for c in edge.WIDE_CHUNKS + (6,):
        assert classes_over(2 * T + 421, 2 * T + 64 * c) == every, c
    # a tile with one start between two tiles with none
    by_rec = {}
    for t in tiles:
        by_rec.setdefault(t["record"], []).append(len(t["starts"]))
    assert strands([dict(record=i) for i, n in by_rec.items() if n[1:] == [0, 1, 0]]) == both
    # chains at this tile: one, two and three tiles without a start
    assert set(geometry(f, T, detail=False)["chains"]) >= {1, 2, 3}


def test_chains_cross_the_scans_blocks():
    f = edge.fixture("chains")
    C = edge.CHAIN_TILES
    assert edge.SCAN_BLOCK == 6144 and C >= 3 * edge.SCAN_BLOCK
    assert not f["model"][2].any() and len(f["records"]) == 10 + sum(edge.CHAIN_LEAD[i % 4] for i in range(10))
    long_ = sorted(f["fx"].cases)
    assert [f["fx"].cases[i] for i in long_] == [(p, s) for p in ("none", "all", "last", "middle", "tile end") for s in "+-"]
    assert all(int(f["ops"][int(f["records"][i]["cigar_off"])]) == 4 << 29 | edge.CHAIN_BASES for i in long_)
    for tile, least in ((64, C), (1024, C // 16)):
        g = geometry(f, tile, detail=False)
        per = {}  # the chains of each long record, in order
        one = {i: edge.geometry(f["records"][i:i + 1], f["ops"], [0], {(0, 0): f["masks"][(i, 0)]}, tile, detail=False)["chains"] for i in long_}
        assert sorted(sum(one.values(), [])) == sorted(g["chains"])
        for i in long_:
            per.setdefault(f["fx"].cases[i][0], set()).add(tuple(one[i]))
        n = edge.CHAIN_BASES // tile
        assert max(g["chains"]) >= least
        assert per["none"] == per["all"] == {(n - 1,)} and n - 1 >= least
        assert per["last"] == {(n - 2,)}                       # ... the last tile has the start at the op's last position
        assert per["middle"] == {(n // 2 - 1, n - n // 2 - 1)} and min(per["middle"].pop()) > edge.SCAN_BLOCK // (tile // 64)
        end = (C + 16) * 64 // tile  # the tile that the X run starts: the '=' run ends with the tile before it, at both sizes
        assert (C + 16) * 64 % tile == 0 and per["tile end"] == {tuple(x for x in (end - 1, n - end - 1) if x)}
        # the place of each long record's first item among the blocks' four waves
        first, at = [], 0
        for i in range(len(f["records"])):
            if i in one:
                first.append(at % 4)
            at += n if i in one else 1
        assert set(first) == {0, 1, 2, 3}


def test_checked_counts_its_lies_and_copies_its_pool():
    f = edge.fixture("checked")
    out_rec, out, flags, rep = f["model"]
    fx = f["fx"]
    assert not flags.any() and out.tolist() == f["ops"].tolist() and out_rec.tobytes() == f["records"].tobytes()
    assert rep["m_ops"] == 0 and rep["ops_in"] == rep["ops_out"] == len(f["records"])
    lies = {"=": 0, "X": 0}
    for case in fx.cases.values():
        lies[case[3]] += case[5]
    assert (rep["bad_eq_bases"], rep["bad_x_bases"]) == (lies["="], lies["X"]) == (fx.planted["bad_eq"], fx.planted["bad_x"])
    assert lies["="] > 100 and lies["X"] > 2 * 1024
    for i, case in fx.cases.items():  # the lies are where the case says: counted from the mask
        d = f["masks"][(i, 0)]
        assert int((d if case[3] == "=" else ~d).sum()) == case[5]
    for T in edge.CHECKED_TILES:
        tiles = [t for t in geometry(f, T)["tiles"] if fx.cases[t["record"]][0] == T]
        for code in (0, 1):
            for strand in "+-":
                mine = [t for t in tiles if t["code"] == code and fx.cases[t["record"]][4] == strand]
                lies_at = set()  # (tile k, position in the tile, the tile's bases) of every lie of a record with at most two
                for t in mine:
                    d = f["masks"][(t["record"], 0)]
                    if fx.cases[t["record"]][5] <= 2:
                        lie = np.flatnonzero((d if code == 0 else ~d)[t["k"] * T:t["k"] * T + t["bases"]])
                        lies_at |= {(t["k"], p, t["bases"]) for p in lie.tolist()}
                what = (T, code, strand)
                assert {k for k, _, _ in lies_at} == {0, 1, 2}, what                                  # tiles behind the first
                assert (0, 0, T) in lies_at and {(0, T - 1, T), (1, 0, T)} <= lies_at, what           # the op's first position; both sides of a tile border
                assert [1 for k, p, n in lies_at if p == n - 1 and n < T] and [1 for k, p, n in lies_at if p == n - 1 and n == 1], what  # its last
                if T > 64:  # both sides of a chunk border inside a tile
                    assert [1 for k, p, n in lies_at if p % 64 == 63 and p + 1 < n] and [1 for k, p, n in lies_at if p % 64 == 0 and p], what
                assert [1 for k, p, n in lies_at if k == 2 and n % 64 and n - n % 64 < p < n - 1], what  # inside a partial last chunk
    whole = [c for c in fx.cases.values() if c[2] in ("all", "none") and c[1] > 2 * 1024]
    assert (1024, 2057, "all", "X", "+", 2057) in whole and (1024, 3072, "none", "=", "-", 0) in whole


def test_holes_are_where_the_searches_meet_them():
    f = edge.fixture("holes")
    recs, flags = f["records"], f["model"][2]
    assert (recs["cigar_len"] == 0).astype(int).tolist() == edge.HOLES_EMPTY and flags.tolist() == edge.HOLES_FLAGS
    assert edge.HOLES_EMPTY[0] and edge.HOLES_EMPTY[-1] and edge.HOLES_EMPTY[2:5] == [1, 1, 1]
    ops_of = lambda i: f["ops"][int(recs[i]["cigar_off"]):int(recs[i]["cigar_off"]) + int(recs[i]["cigar_len"])].tolist()
    assert ops_of(5) == [4 << 29 | 4096] and ops_of(6) == [] and ops_of(7) == [4 << 29 | 1]
    assert ops_of(9) == [4 << 29 | 5000] and flags[8] == flags[10] == 0 and len(ops_of(8)) == len(ops_of(10)) == 3
    out_rec, out = f["model"][0], f["model"][1]
    assert out[int(out_rec[9]["cigar_off"]):int(out_rec[9]["cigar_off"]) + int(out_rec[9]["cigar_len"])].tolist() == [4 << 29 | 5000]
    for tile in (64, 1024, 4096):  # the flagged op is one item at every size
        g = geometry(f, tile)
        assert not [t for t in g["tiles"] if t["record"] == 9]
        assert g["items"] == 1 + sum(max(1, -(-(int(w) & ref.LEN_MASK) // tile)) if int(w) >> 29 != 2 and int(w) >> 29 != 3 else 1
                                     for i in range(len(recs)) if i != 9 for w in ops_of(i))


def test_item_counts_tell_the_tiles_apart():
    """what the device test of the tile size leans on: no two of the sizes it runs cut a fixture into the same number of items"""
    for name in ("wide", "checked", "holes"):
        f = edge.fixture(name)
        n = [geometry(f, t, detail=False)["items"] for t in (64, 256, 1024, 2048, 4096)]
        assert len(set(n)) == len(n), (name, n)


def test_shipped_world_and_its_ranges():
    """the end-to-end world of the device tests: resolvable throughout, cut at 1024, its ranges where the docstring says"""
    f = edge.shipped()
    recs, rl = f["records"], f["ranges"]
    assert not f["model"][2].any() and (recs["cigar_len"] == 1).all() and f["names"] == ["Q1024", "T", "QC1024", "C", "QCw"]
    host = impg_amd.resolve_cigars(recs, f["ops"], f["names"], f["seq_len"], sequences(f["store"]), on_host=True)
    same(host, f["model"], "shipped")
    rep = f["model"][3]
    assert rep["m_ops"] == sum(len(edge.wide_patterns(1024, L)) for L in edge.wide_lengths(1024)) * 2 and rep["bad_eq_bases"] and rep["bad_x_bases"] > 2 * 1024
    g = geometry(f, 1024)
    assert max(t["k"] for t in g["tiles"] if t["code"] == 4) == 3 and max(t["k"] for t in g["tiles"] if t["code"] < 2) == 2
    assert len(rl) == 40 and all(0 <= s < e <= f["seq_len"][t] for t, s, e in rl)
    inside = lambda t, p: [i for i, r in enumerate(recs) if r["target_id"] == t and r["target_start"] <= p < r["target_end"]]
    assert all(inside(t, s) for t, s, e in rl) and {t for t, s, e in rl} == {f["names"].index("T"), f["names"].index("C")}
    second = ends_in_crossing = 0
    for t, s, e in rl:
        for i in inside(t, s):
            second += 1024 <= s - int(recs[i]["target_start"]) < 2048
        for i in inside(t, e - 1):
            d, p = f["masks"][(i, 0)], e - 1 - int(recs[i]["target_start"])
            if int(f["ops"][int(recs[i]["cigar_off"])]) >> 29 == 4 and 1024 <= p < len(d) - 1:
                ends_in_crossing += bool((d[1023:p + 2] == d[p]).all())  # the run goes on behind the range's end and began before the border
    assert second and ends_in_crossing
