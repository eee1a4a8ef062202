"""Every result form of a batch against the oracle, and which projection kernel ran it (tests/test_gpu_projection_paths.py).

Run as a script it is the child process of test_gpu_projection_paths.py::test_edge_fixtures_through_every_arm: the
projection switches (IMPG_STAGE_DENSITY, IMPG_ENTRY_MAJOR, IMPG_ORD_ENTRIES) are read once per process, so each setting
gets a fresh process.  The child rebuilds the edge fixtures, compares every form with the oracle, and checks that the
kernel its setting forces actually ran:

  python tests/proj_worker.py <setting>      setting: density0 | density_off | no_entry_major | ord_entries
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import impg_amd  # noqa: E402

ARMS = ["project_lane_levels", "project_staged_levels", "project_staged_rows_levels", "project_entries_slots_levels",
        "project_entries_qs_levels", "project_entries_rows_levels", "project_entries_ident_levels", "project_tp_levels"]
ENTRIES = [a for a in ARMS if a.startswith("project_entries_")]
FORMS = ("stats", "attributed", "ordered", "slots", "batch")
HOLE = np.uint32(0xFFFFFFFF)

# the setting of each child: its one environment variable, and what must (not) have run
SETTINGS = {
    "density0": ("IMPG_STAGE_DENSITY", "0"),      # every level dense
    "density_off": ("IMPG_STAGE_DENSITY", "-1"),  # no level dense
    "no_entry_major": ("IMPG_ENTRY_MAJOR", "0"),  # dense fused levels on project_staged_kernel
    "ord_entries": ("IMPG_ORD_ENTRIES", "1"),     # ordered rows of a dense fused level entry by entry
}


def snapshot(g):
    return {a: g.counter(a) for a in ARMS}


def delta(g, before):
    now = snapshot(g)
    return {a: now[a] - before[a] for a in ARMS if now[a] != before[a]}


def oracle_answers(c, ranges, kw, cache=None):
    """The oracle's rows of every range (self interval first) and the sum of its last_projection_count()."""
    key = tuple(sorted(kw.items()))
    want, n_proj = [], 0
    for r in ranges:
        k = (key, tuple(r))
        hit = cache.get(k) if cache is not None else None
        if hit is None:
            hit = (c.query(*r, **kw), c.last_projection_count())
            if cache is not None:
                cache[k] = hit
        want.append(hit[0])
        n_proj += hit[1]
    return want, n_proj


def _rows_sorted(rng_idx, rows):
    """(range, row) pairs as one int64 matrix in lexicographic order: a multiset per range."""
    m = np.column_stack([rng_idx.astype(np.int64)] + [rows[f].astype(np.int64) for f in impg_amd.INTERVAL_DTYPE.names])
    if not len(m):
        return m
    return m[np.lexsort(m.T[::-1])]


def attributed_rows(dr, min_output_length=None):
    """The rows of IMPG_ROWS_ATTRIBUTED, attributed through source[] / frontier[] (as _device_rows_by_range in
    test_gpu_parity.py), as a sorted (range, row) matrix."""
    idx, out = [], []
    for k in range(len(dr.parts())):
        first, level, qid, co, src, fr = dr.part_to_host(k)
        live = qid != HOLE
        if min_output_length is not None:
            live &= np.abs(co[:, 1].astype(np.int64) - co[:, 0]) >= min_output_length
        assert (src < len(fr)).all()
        f = fr[src[live]]
        r = np.zeros(int(live.sum()), dtype=impg_amd.INTERVAL_DTYPE)
        r["query_id"], r["q_first"], r["q_last"] = qid[live], co[live, 0], co[live, 1]
        r["target_id"], r["t_first"], r["t_last"] = f["target_id"], co[live, 2], co[live, 3]
        idx.append(first + f["range_idx"].astype(np.int64))
        out.append(r)
    if not out:
        return _rows_sorted(np.zeros(0, np.int64), np.zeros(0, dtype=impg_amd.INTERVAL_DTYPE))
    return _rows_sorted(np.concatenate(idx), np.concatenate(out))


def check_forms(g, c, ranges, kw, forms=FORMS, cache=None, device_ranges=None, expect=None, tag=""):
    """Runs `ranges` under `kw` in every form of `forms` and compares each with the oracle:
      stats       query_batch_stats: per-range counts and checksums, projected
      attributed  query_batch_device, IMPG_ROWS_ATTRIBUTED: the multiset of rows per range, counts / checksums from HBM
      ordered     query_batch_device, IMPG_ROWS_ORDERED: the oracle's rows in the oracle's order
      slots       query_batch_device, IMPG_ROWS_ORDERED_SLOTS: the same, with the hole rows taken out
      batch       query_batch: the same, on the host
    device_ranges: a torch tensor holding the same ranges in HBM; the stats and device forms then take them from there.
    expect: {form: counter name} -- the projection kernel that form must have run (its counter rose).
    Returns {form: {counter: rise}}."""
    from tests.test_gpu_fullsize import checksum
    p = impg_amd.make_params(**kw)
    want, n_proj = oracle_answers(c, ranges, kw, cache)
    n = len(ranges)
    lens = np.array([len(w) for w in want], dtype=np.int64)
    W = np.concatenate(want) if n else np.zeros(0, dtype=impg_amd.INTERVAL_DTYPE)
    woff = np.concatenate([[0], np.cumsum(lens)])
    hits = [w[1:] for w in want]
    want_ck = np.array([checksum(h) for h in hits], dtype=np.uint64)
    dev = {} if device_ranges is None else dict(device_ptr=device_ranges.data_ptr(), n=n)
    mol = kw.get("min_output_length") if kw.get("transitive") else None
    arms = {}
    for form in forms:
        what = (tag, kw, form)
        before = snapshot(g)
        if form == "stats":
            st, cnt, ck = g.query_batch_stats(None if dev else ranges, p, **dev)
            assert st.projected == n_proj, what
            assert (cnt.astype(np.int64) == lens - 1).all(), (what, np.nonzero(cnt.astype(np.int64) != lens - 1)[0][:8])
            assert (ck == want_ck).all(), (what, np.nonzero(ck != want_ck)[0][:8])
            arms[form] = delta(g, before)
            arms[form]["_pairs"] = int(st.pairs)
        elif form == "attributed":
            dr = g.query_batch_device(None if dev else ranges, p, **dev)
            arms[form] = delta(g, before)
            assert dr.projected == n_proj, what
            cnt, ck = dr.check()
            assert (cnt.astype(np.int64) == lens - 1).all() and (ck == want_ck).all(), what
            got = attributed_rows(dr, mol)
            ridx = np.repeat(np.arange(n, dtype=np.int64), lens - 1)
            exp = _rows_sorted(ridx, np.concatenate(hits) if n else W)
            assert got.shape == exp.shape and (got == exp).all(), what
            dr.free()
        elif form in ("ordered", "slots"):
            layout = impg_amd._lib.ROWS_ORDERED if form == "ordered" else impg_amd._lib.ROWS_ORDERED_SLOTS
            do = g.query_batch_device(None if dev else ranges, p, layout=layout, **dev)
            arms[form] = delta(g, before)
            assert do.projected == n_proj, what
            seen = 0
            for k in range(len(do.parts())):
                first, rows, off = do.ordered_to_host(k)
                off = off.astype(np.int64)
                if form == "slots":  # the hole rows out, the offsets with them
                    keep = rows["query_id"] != HOLE
                    off = np.concatenate([[0], np.cumsum(keep)])[off]
                    rows = rows[keep]
                m = len(off) - 1
                assert (np.diff(off) == lens[first:first + m]).all(), (what, first)
                assert (rows[off[0]:off[-1]] == W[woff[first]:woff[first + m]]).all(), (what, first)
                seen += m
            assert seen == n, what
            do.free()
        elif form == "batch":
            res = g.query_batch(ranges, p)
            arms[form] = delta(g, before)
            assert res.projected == n_proj, what
            assert (res.offsets.astype(np.int64) == woff).all(), what
            assert (res.intervals == W).all(), what
        else:
            raise ValueError(form)
        if expect and form in expect:
            assert arms[form].get(expect[form], 0) > 0, (what, "expected %s" % expect[form], arms[form])
    return arms


def build_index(d, text, bidirectional=True):
    from oracle import oracle as o
    path = os.path.join(d, "f%d.paf" % len(os.listdir(d)))
    with open(path, "w") as f:
        f.write(text)
    g = impg_amd.GpuImpg.from_paf(path, bidirectional=bidirectional)
    c = o.OracleIndex(paf_paths=[path], bidirectional=bidirectional, preparse=True)
    return g, c


def dense_tiling(g, ranges, per_entry=40.0):
    """The ranges repeated until a plain level holds >= per_entry pairs per index entry (a dense level by the default
    thresholds), so that the forcing switches have a dense level to act on."""
    st, _, _ = g.query_batch_stats(ranges, impg_amd.make_params(), counts=False, checksums=False)
    need = per_entry * g.num_entries()
    k = max(1, int(np.ceil(need / max(1, st.pairs))))
    return list(ranges) * k


def edge_fixtures():
    """(name, PAF text, ranges(g), kw list) of the edge fixtures: test_prefix_line_edges, the wide last tile under the
    identity filter, and random_paf with weird / inconsistent CIGARs and long records."""
    from tests.paf_gen import random_paf, random_ranges
    from tests.test_gpu_parity import IDENTITY_WIDE_THRESHOLDS, identity_wide_fixture, prefix_line_edges_fixture
    bfs = dict(transitive=True, max_depth=2, min_transitive_len=1, min_distance_between_ranges=0)
    out = []
    text, mk = prefix_line_edges_fixture()
    out.append(("prefix_line_edges", text, mk, [dict(), bfs]))
    text, mk = identity_wide_fixture()
    out.append(("identity_wide_last_tile", text, mk, [dict()] + [dict(min_identity=t) for t in IDENTITY_WIDE_THRESHOLDS[:3]] +
                [dict(bfs, min_identity=0.9999)]))
    for seed, kwp in [(61, dict(weird=True)), (62, dict(weird=True, inconsistent=True)), (63, dict(max_ops=1200))]:
        text, _ = random_paf(seed, 500, **kwp)
        mk = (lambda s: lambda g: random_ranges(s + 1, 300, 6, 20000, max_len=6000, min_len=1))(seed)
        out.append(("random_paf_%d" % seed, text, mk, [dict(), dict(bfs, max_depth=2, min_transitive_len=20), dict(min_identity=0.8)]))
    return out


def short_ranges(g):
    """Ranges of <= 60 bp over random_paf's records: one or two pairs each over a span of hundreds of entries -- the
    blocks project_entries_kernel takes a lane per place (its sparse branch) once the level counts as dense."""
    from tests.paf_gen import random_ranges
    return random_ranges(5, 400, 6, 20000, max_len=60, min_len=1)


def run_setting(setting):
    var, val = SETTINGS[setting]
    assert os.environ.get(var) == val, "the parent sets %s=%s" % (var, val)
    total = {a: 0 for a in ARMS}
    with tempfile.TemporaryDirectory() as d:
        for name, text, mk, kws in edge_fixtures():
            g, c = build_index(d, text)
            g.set_option("locality_min", 1)
            g.set_option("fuse_final_level", 1)
            g.set_option("walk_kernel", 0)  # (the small BFS batches stay on the batch engine's projection kernels)
            sets = [dense_tiling(g, mk(g))]
            if setting == "density0" and name.startswith("random_paf"):  # (every level dense: sparse blocks too)
                sets.append(short_ranges(g))
            cache = {}
            before = snapshot(g)
            for ranges in sets:
                for kw in kws:
                    check_forms(g, c, ranges, kw, cache=cache, tag=(setting, name, len(ranges)))
            for a, v in delta(g, before).items():
                total[a] += v
            print("%s %s: %s ranges, arms %s" % (setting, name, [len(r) for r in sets], delta(g, before)), flush=True)
    others = lambda keep: {a: v for a, v in total.items() if v and a not in keep}
    if setting == "density0":
        assert total["project_entries_slots_levels"] > 0 and total["project_entries_qs_levels"] > 0, total
        assert total["project_staged_levels"] > 0 and total["project_staged_rows_levels"] > 0, total
        assert total["project_entries_ident_levels"] > 0, total
    elif setting == "density_off":
        assert total["project_lane_levels"] > 0 and not others({"project_lane_levels"}), total
    elif setting == "no_entry_major":
        assert total["project_staged_levels"] > 0 and not any(total[a] for a in ENTRIES), total
    elif setting == "ord_entries":
        assert total["project_entries_rows_levels"] > 0 and total["project_staged_rows_levels"] == 0, total
    print("proj_worker %s ok: %s" % (setting, {a: v for a, v in total.items() if v}), flush=True)


if __name__ == "__main__":
    run_setting(sys.argv[1])
