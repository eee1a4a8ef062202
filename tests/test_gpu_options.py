"""impg_gpu_set_option / impg_gpu_get_counter as tables (csrc/options.hpp): every key's range as the if / else chain had
it, every counter readable, answers unchanged by a round trip through the options, and a multi-GPU handle handing its
options to its ranks before each of its four batch forms."""
import pytest

import impg_amd
from oracle import oracle as o
from tests.paf_gen import random_paf, random_ranges
from tests.test_gpu_fullsize import checksum
from tests.test_gpu_parity import _device_rows_by_range

pytestmark = pytest.mark.gpu

I64_MAX = 2 ** 63 - 1
# (key, lowest, highest accepted value) of every ranged option, from the chain in capi.cpp before the table; None: no
# upper limit below the int64 the ABI takes
RANGED = [("pair_budget", 1024, 0xFFFFFFF0 - 1), ("chunk_ranges", 0, 2 ** 31 - 1), ("locality_min", 0, 2 ** 31 - 1),
          ("device_rows_pool_bytes", 0, None), ("walk_kernel", 0, 2), ("segment_parts", 0, 4096), ("walk_members", 0, 64),
          ("filter_covered", 0, 2), ("wide_emit_cap", 64, 4096), ("wide_emit_bins", 2, 1024), ("approximate_cigar", 0, 1),
          ("debug_fail_owner", 0, 0xFFFFFFFF), ("debug_fail_home", 0, 0xFFFFFFFF), ("lane_schedule", 0, None),
          ("bed_text_piece_bytes", 64, 2 ** 40), ("prewarm_result_bytes", 0, None), ("prewarm_walk", 0, 2)]
# accepting their upper end allocates gigabytes (pinned host memory, walk slabs, the rows pool's cap): 0 and 1 only
NO_HIGH_END = ("prewarm_result_bytes", "prewarm_walk", "device_rows_pool_bytes")
FLAGS = ["fuse_final_level", "regroup_entries", "segment_groups", "update_stats", "lookup_stats", "free_slot_order"]
# every stored option: (default, another value in range)
STORED = {"pair_budget": (1 << 28, 4096), "chunk_ranges": (0, 3), "locality_min": (4096, 1), "device_rows_pool_bytes": (160 << 30, 1 << 20),
          "fuse_final_level": (1, 0), "regroup_entries": (1, 0), "walk_kernel": (1, 0), "segment_groups": (1, 0), "segment_parts": (0, 2),
          "walk_members": (0, 1), "filter_covered": (0, 1), "update_stats": (0, 1), "lookup_stats": (0, 1), "wide_emit_cap": (4096, 64),
          "wide_emit_bins": (1024, 2), "approximate_cigar": (0, 1), "free_slot_order": (1, 0), "debug_fail_owner": (0, (1 << 16) | 1),
          "debug_fail_home": (0, (1 << 16) | 1), "lane_schedule": (0, 1), "bed_text_piece_bytes": (256 << 20, 64)}
BFS = dict(transitive=True, max_depth=3, min_transitive_len=20)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """one tiny alignment file, its oracle, a batch of ranges and the oracle's rows for a plain and a transitive query"""
    text, _ = random_paf(77, 60, n_seq=5, seq_len=20000, self_aln=True)
    path = str(tmp_path_factory.mktemp("options") / "w.paf")
    with open(path, "w") as f:
        f.write(text)
    c = o.OracleIndex(paf_paths=[path], preparse=True)
    rl = random_ranges(100, 24, c.num_seqs(), 20000, max_len=3000, min_len=120)
    want = {name: [c.query(t, s, e, **kw) for (t, s, e) in rl] for name, kw in (("plain", dict()), ("bfs", BFS))}
    return path, c, rl, want


def lists(rows):
    return [r.tolist() for r in rows]


def refused(g, key, value):
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        g.set_option(key, value)
    assert ei.value.code == impg_amd.IMPG_E_INVALID, (key, value)


def test_option_ranges(world):
    g = impg_amd.GpuImpg.from_paf(world[0])
    assert {k for k, _, _ in RANGED} | set(FLAGS) == set(STORED) | {"prewarm_result_bytes", "prewarm_walk"}
    for key, lo, hi in RANGED:
        refused(g, key, lo - 1)
        if hi is not None:
            refused(g, key, hi + 1)
        refused(g, key, -I64_MAX - 1)
        accept = [0, 1] if key in NO_HIGH_END else [lo, hi if hi is not None else I64_MAX]
        for v in accept:
            g.set_option(key, v)
        if key in STORED:
            g.set_option(key, STORED[key][0])
    for key in FLAGS:  # stored as value != 0: any integer is accepted
        for v in (0, 1, 7, -1, I64_MAX):
            g.set_option(key, v)
        g.set_option(key, STORED[key][0])
    refused(g, "approximate_cigar", 2)
    refused(g, "no_such_option", 0)
    with pytest.raises(impg_amd.ImpgGpuError) as ei:
        g.counter("no_such_counter")
    assert ei.value.code == impg_amd.IMPG_E_INVALID


def test_every_counter_reads(world):
    g = impg_amd.GpuImpg.from_paf(world[0])
    keys = impg_amd.counter_keys()
    assert len(keys) >= 31 and {"build_device", "tokenized_device", "build_batches"} <= set(keys)
    for key in keys:
        assert g.counter(key) >= 0, key
    assert [g.counter(k) for k in ("build_device", "tokenized_device", "build_batches")] == [1, 1, 1]  # from_paf, one tiles launch
    m = impg_amd.GpuImpg.from_paf(world[0], devices=[0, 0], lanes=1)  # a multi handle: the sum over its ranks
    assert [m.counter(k) for k in ("build_device", "tokenized_device", "build_batches")] == [2, 0, 2]


def test_same_answers_after_an_options_round_trip(world):
    path, c, rl, want = world
    g = impg_amd.GpuImpg.from_paf(path)

    def rows(kw):
        got = g.query_batch(rl, impg_amd.make_params(**kw))
        return [got[i].tolist() for i in range(len(rl))]

    assert rows(dict()) == lists(want["plain"]) and rows(BFS) == lists(want["bfs"])
    for key, (default, other) in STORED.items():
        g.set_option(key, other)
    for key, (default, other) in STORED.items():
        g.set_option(key, default)
    assert rows(dict()) == lists(want["plain"]) and rows(BFS) == lists(want["bfs"])


def test_every_batch_form_forwards(world):
    """A multi handle hands debug_fail_owner -- the host-side failure injection of test_failure_agreement_multi_handle -- to
    its ranks before a full-results, a counting, a BED and a device-rows batch alike; with the option back at 0 each form
    answers as the oracle does."""
    path, c, rl, want = world
    g = impg_amd.GpuImpg.from_paf(path, devices=[0, 0], lanes=1)
    g.set_option("chunk_ranges", 7)  # two chunks a rank
    p = impg_amd.make_params(**BFS)
    forms = {"results": lambda: g.query_batch(rl, p), "stats": lambda: g.query_batch_stats(rl, p),
             "bed": lambda: g.query_batch_bed(rl, p, merge_distance=100), "device rows": lambda: g.query_batch_device(rl, p)}
    g.set_option("debug_fail_owner", (1 << 16) | 1)  # rank 0, the batch's first hop
    for name, form in forms.items():
        with pytest.raises(impg_amd.ImpgGpuError) as ei:
            form()
        assert "injected failure" in str(ei.value), (name, str(ei.value))
    g.set_option("debug_fail_owner", 0)
    got = forms["results"]()
    assert [got[i].tolist() for i in range(len(rl))] == lists(want["bfs"])
    st, cnt, ck = forms["stats"]()
    assert cnt.tolist() == [len(w) - 1 for w in want["bfs"]]
    assert [int(x) for x in ck] == [checksum(w[1:]) for w in want["bfs"]]
    assert forms["bed"]() == "".join(c.query_bed(c.seq_name(t), s, e, merge_distance=100, **BFS) for (t, s, e) in rl)
    dr = forms["device rows"]()
    by_range = _device_rows_by_range(dr, len(rl), None)
    dr.free()
    for i in range(len(rl)):
        assert sorted(by_range[i]) == sorted(tuple(int(x) for x in r) for r in want["bfs"][i][1:].tolist()), i
