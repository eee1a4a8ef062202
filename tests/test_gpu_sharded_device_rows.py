"""impg_gpu_query_batch_device on a sharded index (multi-GPU handles here; the shards share device 0): levels whose hits
come home stay with the home rank, the final level stays with the rank that projected it, and every row is attributed
to its range of the collective batch.  Compared with the oracle and with a single-GPU index on the same alignments."""
import os
import subprocess
import sys

import numpy as np
import pytest

import impg_amd
from impg_amd import _lib
from impg_amd.index import HOP_PROFILE_FIELDS
from oracle import oracle as o
from tests.paf_gen import random_ranges
from tests.test_gpu_parity import _device_rows_by_range
from tests.test_multi_gpu import lane_cases, write_paf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the parameter cases of test_device_rows_attributed: plain, BFS -m 1 and -m 3, -m 0 with min_output_length, min_identity
KWS = [dict(), dict(transitive=True, max_depth=1, min_transitive_len=20),
       dict(transitive=True, max_depth=3, min_transitive_len=20, min_distance_between_ranges=0),
       dict(transitive=True, max_depth=0, min_transitive_len=30, min_output_length=60),
       dict(transitive=True, max_depth=3, min_identity=0.7)]
BYTES_HITS_OUT = HOP_PROFILE_FIELDS.index("bytes_hits_out")


def oracle_rows(c, ranges, kw):
    want, n_proj = [], 0
    for (t, s, e) in ranges:
        want.append(sorted(tuple(int(x) for x in r) for r in c.query(t, s, e, **kw)[1:].tolist()))
        n_proj += c.last_projection_count()
    return want, n_proj


def check_rows(g, single, c, ranges, kw, devices, want=None, n_proj=None):
    """one query_batch_device call on g against the oracle and the single-GPU counting form"""
    if want is None:
        want, n_proj = oracle_rows(c, ranges, kw)
    p = impg_amd.make_params(**kw)
    dr = g.query_batch_device(ranges, p)
    st, cnt, ck = single.query_batch_stats(ranges, p)
    assert dr.projected == n_proj == st.projected, (kw, dr.projected, n_proj)
    cnt2, ck2 = dr.check()
    assert (cnt2 == cnt).all() and (ck2 == ck).all(), kw
    assert dr.batch_offset() == (0, len(ranges))
    for k in range(len(dr.parts())):
        assert dr.part_device(k) in devices
    got = _device_rows_by_range(dr, len(ranges), kw.get("min_output_length") if kw.get("transitive") else None)
    for i in range(len(ranges)):
        assert sorted(got[i]) == want[i], (kw, i)
    dr.free()


def schedules(world, lanes):
    """lane_schedule 0 and the first two forced hand-over patterns where there are several lanes"""
    return [s for (_, _, s) in lane_cases([(world, lanes)])][:3]


@pytest.mark.parametrize("world,lanes", [(1, 1), (2, 1), (3, 2), (5, 3), (8, 2)])
def test_sharded_device_rows_match_oracle(tmp_path, world, lanes):
    path = write_paf(tmp_path)
    c = o.OracleIndex(paf_paths=[path], preparse=True)
    g = impg_amd.GpuImpg.from_paf(path, devices=[0] * world, lanes=lanes)
    single = impg_amd.GpuImpg.from_paf(path)
    g.set_option("chunk_ranges", 7)  # many chunks: every lane is used, ranks run different numbers of real chunks
    ranges = random_ranges(100, 53, c.num_seqs(), 20000, max_len=3000, min_len=120)
    for kw in KWS:
        want, n_proj = oracle_rows(c, ranges, kw)
        for sched in schedules(world, lanes):
            g.set_option("lane_schedule", sched)
            check_rows(g, single, c, ranges, kw, [0], want, n_proj)
        g.set_option("lane_schedule", 0)
        if world > 1:  # the listed final level and the frontier order of small levels, too
            for lm, fuse in [(1, 0), (4096, 0), (1, 1), (4096, 1)]:
                g.set_option("locality_min", lm)
                g.set_option("fuse_final_level", fuse)
                check_rows(g, single, c, ranges, kw, [0], want, n_proj)
            g.set_option("locality_min", 4096)
            g.set_option("fuse_final_level", 1)


def test_sharded_device_rows_stay_on_owners(tmp_path):
    """The final hop of a rows batch sends nothing home (its hits stay where they were projected); the full-results form
    of the same batch does ship them."""
    path = write_paf(tmp_path)
    c = o.OracleIndex(paf_paths=[path], preparse=True)
    g = impg_amd.GpuImpg.from_paf(path, devices=[0, 0, 0], lanes=1)
    ranges = random_ranges(7, 40, c.num_seqs(), 20000, max_len=3000, min_len=120)
    kw = dict(transitive=True, max_depth=2, min_transitive_len=20)
    p = impg_amd.make_params(**kw)
    g.hop_profile(reset=True)
    dr = g.query_batch_device(ranges, p)
    prof = g.hop_profile(reset=True)
    assert dr.projected > 0
    assert (prof[:, 0, 0] == 1).all() and (prof[:, 1, 0] == 1).all() and (prof[:, 2:, 0] == 0).all()  # one chunk, two hops
    assert (prof[:, 0, BYTES_HITS_OUT] > 0).any()  # level 0 comes home for the visited-set update
    assert (prof[:, 1, BYTES_HITS_OUT] == 0).all()  # the final level does not
    dr.free()
    g.query_batch(ranges, p)
    prof = g.hop_profile(reset=True)
    assert (prof[:, 1, BYTES_HITS_OUT] > 0).any()


def test_sharded_device_rows_edges(tmp_path):
    path = write_paf(tmp_path, seed=5, n=400)
    c = o.OracleIndex(paf_paths=[path], preparse=True)
    single = impg_amd.GpuImpg.from_paf(path)
    g = impg_amd.GpuImpg.from_paf(path, devices=[0, 0, 0], lanes=2)
    kw = dict(transitive=True, max_depth=3, min_transitive_len=30)
    # an empty batch
    dr = g.query_batch_device([], impg_amd.make_params(**kw))
    assert dr.projected == 0 and len(dr.parts()) == 0 and dr.batch_offset() == (0, 0)
    cnt, ck = dr.check()
    assert cnt.size == 0 and ck.size == 0
    dr.free()
    # fewer ranges than ranks: some ranks have none of their own, but still serve as owners
    rl = random_ranges(9, 300, c.num_seqs(), 20000, max_len=6000, min_len=500)
    for kw2 in (dict(), kw):
        check_rows(g, single, c, rl[:2], kw2, [0])
    # ranges that overlap nothing anywhere (beyond every sequence's last alignment) mixed with ranges that do
    far = [(i % 7, 19990, 20000) if i % 2 else rl[i] for i in range(20)]
    for kw2 in (dict(), kw):
        check_rows(g, single, c, far, kw2, [0])
    check_rows(g, single, c, [(i % 7, 19990, 20000) for i in range(5)], kw, [0])
    # owners expand what arrives in slices under the pair budget: one part per slice
    g.set_option("pair_budget", 1024)
    dr = g.query_batch_device(rl, impg_amd.make_params(**kw))
    final = [d for d in dr.parts() if d.first_range == 0 and d.n_ranges == len(rl) and d.level == 2]
    assert len(final) > 3, len(final)
    dr.free()
    check_rows(g, single, c, rl, kw, [0])
    check_rows(g, single, c, rl, dict(), [0])
    g.set_option("pair_budget", 1 << 28)
    # every lane's engine has just run in the rows mode (the final level left with its owners): a full-results call on the
    # same engines brings every final-level hit home -- on this handle, and on one of two ranks x two lanes
    g2 = impg_amd.GpuImpg.from_paf(path, devices=[0, 0], lanes=2)
    g2.set_option("pair_budget", 1024)
    g2.query_batch_device(rl, impg_amd.make_params(**kw)).free()
    g2.set_option("pair_budget", 1 << 28)
    for h in (g, g2):
        for kw2 in (dict(), kw):
            h.query_batch_device(rl, impg_amd.make_params(**kw2)).free()  # (rows mode once more, then the rows at home)
            res = h.query_batch(rl, impg_amd.make_params(**kw2))
            for i, (t, s, e) in enumerate(rl):
                assert res[i].tolist() == c.query(t, s, e, **kw2).tolist(), (kw2, i)


def test_sharded_device_rows_tracepoints():
    from tests.tp_gen import random_tp
    d = random_tp(41, 700, n_seq=5, seq_len=60_000)
    c = o.OracleIndex(tracepoints=d)
    kwt = dict(query_deltas=d["query_deltas"], diffs=d["diffs"], fastga=d["fastga"], trace_spacing=d["trace_spacing"],
               max_complexity=d["max_complexity"])
    single = impg_amd.GpuImpg.from_tracepoints(d["records"], d["tracepoints"], d["seq_len"], **kwt)
    g = impg_amd.GpuImpg.from_tracepoints(d["records"], d["tracepoints"], d["seq_len"], devices=[0, 0, 0], lanes=2, **kwt)
    g.set_option("chunk_ranges", 11)
    ranges = random_ranges(41, 60, 5, 60_000, max_len=4000, min_len=1)
    for kw in (dict(), dict(transitive=True, max_depth=3, min_transitive_len=30), dict(min_identity=0.85)):
        check_rows(g, single, c, ranges, kw, [0])


def test_sharded_device_rows_refusals(tmp_path):
    path = write_paf(tmp_path)
    g = impg_amd.GpuImpg.from_paf(path, devices=[0, 0], lanes=2)
    ranges = [(0, 100, 2000), (1, 500, 900)]
    bfs = impg_amd.make_params(transitive=True, max_depth=2)
    for layout in (_lib.ROWS_ORDERED, _lib.ROWS_ORDERED_SLOTS):
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            g.query_batch_device(ranges, bfs, layout=layout)
        assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED and "sharded" in str(ei.value)
    for kw in (dict(transitive=True, dfs=True, max_depth=2), dict(transitive=True, max_depth=2, multi_impg=True), dict(store_cigar=True)):
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            g.query_batch_device(ranges, impg_amd.make_params(**kw))
        assert ei.value.code == impg_amd.IMPG_E_UNSUPPORTED and "sharded" in str(ei.value), kw
    import torch
    dev = torch.from_numpy(impg_amd.GpuImpg._ranges(ranges).view(np.uint8)).to("cuda:0")
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        g.query_batch_device(None, bfs, device_ptr=dev.data_ptr(), n=len(ranges))
    assert ei.value.code == impg_amd.IMPG_E_INVALID


LIFETIME = r"""
import sys
sys.path.insert(0, sys.argv[1])
import impg_amd
from tests.paf_gen import random_ranges
g = impg_amd.GpuImpg.from_paf(sys.argv[2], devices=[0, 0, 0], lanes=2)
g.set_option("chunk_ranges", 7)
p = impg_amd.make_params(transitive=True, max_depth=3, min_transitive_len=20)
batches = [random_ranges(50 + k, 20 + 3 * k, 7, 20000, max_len=3000, min_len=120) for k in range(6)]
for rnd in range(2):
    held = [g.query_batch_device(rl, p) for rl in batches]  # more handles than the index has engines (4)
    first = [h.check() for h in held]
    for rl in batches:
        g.query_batch_stats(rl, p)  # later batches reuse every engine and lane buffer
    for h, rl, (c0, k0) in zip(held, batches, first):
        st, cnt, ck = g.query_batch_stats(rl, p)
        c1, k1 = h.check()
        assert (c1 == c0).all() and (k1 == k0).all() and (c1 == cnt).all() and (k1 == ck).all()
        h.free()
print("lifetime ok")
"""


def test_sharded_device_rows_lifetime(tmp_path):
    """A sharded handle holds no engine lease, lane buffer or pool block: six live handles on an index of four engines
    neither block the next call nor see their rows overwritten by it."""
    path = write_paf(tmp_path)
    r = subprocess.run([sys.executable, "-c", LIFETIME, ROOT, path], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "lifetime ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_sharded_device_rows_poisoned(tmp_path):
    """World 3 x 2 lanes and the edge cases once more with IMPG_POISON: a kept part whose block a later slice, hop or
    chunk reused reads the pattern instead of its rows."""
    if os.environ.get("IMPG_POISON"):
        pytest.skip("already a poisoned run")
    env = dict(os.environ, IMPG_POISON="a5")
    sel = "(match_oracle and 3-2) or edges"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout and "failed" not in r.stdout
