"""Every projection kernel that launch_project can pick, against the oracle -- and proof that each one ran.

launch_project sends a level to project_kernel (a lane per pair), project_staged_kernel (listed dense levels; the ordered
rows of a dense fused level) or project_entries_kernel (a dense fused final level, entry by entry, with its sparse
lane-per-place branch, wide windows, records of more than 8 tiles and heavy blocks cut into slices).  The handle counts the
levels each kernel took (GpuImpg.counter("project_*_levels")); every case here asserts that the kernel it targets ran, so
a case that silently lands on another kernel fails instead of passing on the wrong one."""
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import impg_amd
from tests.paf_gen import random_cigar, random_paf, random_ranges, spans
from tests.proj_worker import ARMS, ENTRIES, SETTINGS, build_index, check_forms, delta, snapshot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 400000
LANE, STAGED, STAGED_ROWS = "project_lane_levels", "project_staged_levels", "project_staged_rows_levels"
ENT_SLOTS, ENT_QS, ENT_ROWS, ENT_IDENT = ENTRIES[0], ENTRIES[1], ENTRIES[2], ENTRIES[3]
assert ENTRIES == [ENT_SLOTS, ENT_QS, ENT_ROWS, ENT_IDENT]
ENT_RANGES, ENT_SLICE_PAIRS, ENT_MAX_SLICES = 512, 32768, 64  # project_entries_kernel's block, slice size and slice cap


def pile(rng, target, n, t_lo, t_hi, queries, min_ops=20, max_ops=60, long_ops=0, long_every=0):
    """n PAF lines on `target` starting in [t_lo, t_hi), both strands, their query sides spread over `queries`;
    every long_every-th record has long_ops ops (more than the 8 tiles project_entries_kernel stages: ORIENT = -1)."""
    lines = []
    for k in range(n):
        n_ops = long_ops if long_every and k % long_every == 0 else int(rng.integers(min_ops, max_ops + 1))
        ops = random_cigar(rng, n_ops)
        td, qd = spans(ops)
        ts = int(rng.integers(t_lo, t_hi))
        q = queries[k % len(queries)]
        qs = int(rng.integers(0, L - qd))
        cg = "".join("%d%s" % (ln, c) for ln, c in ops)
        lines.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%s" %
                     (q, L, qs, qs + qd, "+-"[k % 2], target, L, ts, ts + td, td, td + qd, cg))
    return lines


def covering(g, name, n, lo, hi, seed):
    """n ranges on `name`, each covering all of [lo, hi) (so every record there), ends varied."""
    rng = np.random.default_rng(seed)
    t = g.seq_id(name)
    return [(t, int(rng.integers(max(0, lo - 3000), lo)), int(rng.integers(hi, min(L, hi + 3000)))) for _ in range(n)]


def fused_options(g, **opt):
    g.set_option("locality_min", 1)
    g.set_option("fuse_final_level", 1)
    g.set_option("walk_kernel", 0)  # (small BFS batches stay on the batch engine)
    for k, v in opt.items():
        g.set_option(k, v)


# ---- a. the natural thresholds: 32 pairs per index entry (fused levels), 128 (listed levels) -------------------------------
@pytest.fixture(scope="module")
def threshold_index(tmp_path_factory):
    """40 records on T (one direction: 40 index entries) whose query sides lie on Q0..Q7, and T's identity lines."""
    rng = np.random.default_rng(7)
    text = "\n".join(pile(rng, "T", 40, 10000, 12000, ["Q%d" % i for i in range(8)])) + "\n"
    g, c = build_index(str(tmp_path_factory.mktemp("thr")), text, bidirectional=False)
    assert g.num_entries() == 40
    return g, c


M1 = dict(transitive=True, max_depth=1, min_transitive_len=20, min_distance_between_ranges=0)
M2 = dict(transitive=True, max_depth=2, min_transitive_len=20, min_distance_between_ranges=0)


@pytest.mark.parametrize("regroup,free", [(1, 1), (0, 1), (1, 0)])
def test_density_thresholds(threshold_index, regroup, free):
    """Ranges that each hit all 40 entries: 31 of them make 31 pairs per entry (below the fused threshold of 32: every form
    on project_kernel), 160 make 160 (above it and above the listed threshold of 128: the counting form and the attributed
    rows entry by entry, the ordered slots on project_staged_kernel<OUT_ROWS>, the listed forms on project_staged_kernel).
    Identical answers on both sides, all equal to the oracle.  Without the free slot order nothing is staged."""
    g, c = threshold_index
    fused_options(g, regroup_entries=regroup, free_slot_order=free)
    cache = {}
    for n, dense in [(31, False), (160, True)]:
        ranges = covering(g, "T", n, 9000, 15000, n)
        # (every range covers every record: pairs per entry = ranges)
        st, _, _ = g.query_batch_stats(ranges, impg_amd.make_params(), counts=False, checksums=False)
        assert st.pairs == 40 * n
        dense = dense and free
        plain = dict(stats=ENT_SLOTS, attributed=ENT_QS, slots=STAGED_ROWS, ordered=STAGED, batch=STAGED) if dense else \
            dict.fromkeys(["stats", "attributed", "slots", "ordered", "batch"], LANE)
        arms = check_forms(g, c, ranges, {}, cache=cache, expect=plain, tag=(n, regroup, free))
        if dense:  # (nothing else ran: one level, one kernel)
            assert not any(arms["stats"].get(a) for a in ARMS if a != ENT_SLOTS), arms
        # transitive -m 1: the fused final level is the first one (TRANSITIVE kernels)
        check_forms(g, c, ranges, M1, cache=cache, expect=dict(stats=ENT_SLOTS if dense else LANE, slots=STAGED_ROWS if dense else LANE),
                    forms=("stats", "attributed", "slots", "ordered"), tag=(n, regroup, free))
        # -m 2: the first level is listed (Q0..Q7 have no entries of their own: the second finds nothing)
        check_forms(g, c, ranges, M2, cache=cache, expect=dict(stats=STAGED if dense else LANE),
                    forms=("stats", "attributed", "slots"), tag=(n, regroup, free))
        # the identity filter on the index's identity lines: entry by entry, MODE_IDENT
        for thr in (0.6, 0.97):
            check_forms(g, c, ranges, dict(min_identity=thr), cache=cache, expect=dict(stats=ENT_IDENT if dense else LANE, attributed=ENT_IDENT if dense else LANE),
                        forms=("stats", "attributed", "batch"), tag=(n, regroup, free))
    fused_options(g, regroup_entries=1, free_slot_order=1)


def test_density_threshold_answers_agree(threshold_index):
    """The same 31 ranges below the line and inside a 160-range batch above it: the same rows and counts."""
    g, c = threshold_index
    fused_options(g)
    ranges = covering(g, "T", 160, 9000, 15000, 160)
    a = g.query_batch_stats(ranges[:31], impg_amd.make_params())
    b = g.query_batch_stats(ranges, impg_amd.make_params())
    assert (a[1] == b[1][:31]).all() and (a[2] == b[2][:31]).all()


# ---- b. the sparse and the non-sparse blocks of project_entries_kernel --------------------------------------------------------
@pytest.fixture(scope="module")
def block_index(tmp_path_factory):
    """Bidirectional.  512 records spread along S (one range each: a block of 512 ranges with one pair per spanned entry --
    the sparse branch), and a pile of 24 records on U from Q0..Q3 (both strands, every 4th with 260 ops), which 2048
    ranges on U and 512 on Q0..Q3 (the pile's reversed entries) hit over and over: non-sparse blocks."""
    rng = np.random.default_rng(11)
    lines = []
    for k in range(512):  # one record every 700 bp of S (at most 12 ops of <= 30 bp: no two overlap)
        ops = [(int(rng.integers(1, 31)), "=XID"[int(rng.integers(0, 4))]) for _ in range(int(rng.integers(3, 12)))] + [(5, "=")]
        td, qd = spans(ops)
        ts, qs = 1000 + 700 * k, int(rng.integers(0, L - qd))
        cg = "".join("%d%s" % (ln, c) for ln, c in ops)
        lines.append("V\t%d\t%d\t%d\t%s\tS\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%s" % (L, qs, qs + qd, "+-"[k % 2], L, ts, ts + td, td, td + qd, cg))
    lines += pile(rng, "U", 24, 10000, 11000, ["Q0", "Q1", "Q2", "Q3"], min_ops=20, max_ops=50, long_ops=260, long_every=4)
    g, c = build_index(str(tmp_path_factory.mktemp("blk")), "\n".join(lines) + "\n")
    return g, c


def test_entries_sparse_and_pile_blocks(block_index):
    g, c = block_index
    fused_options(g)
    S, U = g.seq_id("S"), g.seq_id("U")
    rng = np.random.default_rng(5)
    sparse = [(S, 1000 + 700 * k + int(rng.integers(0, 200)), 1000 + 700 * k + int(rng.integers(300, 650))) for k in range(512)]
    heavy = [(U, int(rng.integers(5000, 10000)), int(rng.integers(11000, 30000))) for _ in range(2048)]  # (all 24 records each)
    for q in range(4):  # the pile from its query sides: reversed entries
        qid = g.seq_id("Q%d" % q)
        heavy += [(qid, int(rng.integers(0, L // 2)), int(rng.integers(L // 2, L))) for _ in range(128)]
    ranges = sparse + heavy
    st, _, _ = g.query_batch_stats(ranges, impg_amd.make_params(), counts=False, checksums=False)
    assert st.pairs >= 32 * g.num_entries(), (st.pairs, g.num_entries())  # a dense level: the entries kernel
    cache = {}
    check_forms(g, c, ranges, {}, cache=cache, expect=dict(stats=ENT_SLOTS, attributed=ENT_QS, slots=STAGED_ROWS), tag="blocks")
    check_forms(g, c, ranges, M1, cache=cache, expect=dict(stats=ENT_SLOTS), forms=("stats", "attributed"), tag="blocks")
    check_forms(g, c, ranges, dict(min_identity=0.9), cache=cache, expect=dict(stats=ENT_IDENT), forms=("stats", "attributed"), tag="blocks")
    # the sparse block alone (a level of 512 pairs is not dense: project_kernel) and the pile alone
    check_forms(g, c, sparse, {}, cache=cache, expect=dict(stats=LANE), forms=("stats",), tag="sparse alone")
    check_forms(g, c, heavy[:2048], {}, cache=cache, expect=dict(stats=ENT_SLOTS, attributed=ENT_QS), forms=("stats", "attributed"), tag="pile")


# ---- c. heavy blocks cut into slices ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rec,n_ranges,slices", [(100, 400, 2), (600, 500, 10), (5000, 512, 64)])
def test_entries_heavy_block_slices(tmp_path, n_rec, n_ranges, slices):
    """One block of <= 512 ranges, non-transitive (the final level is that one block), over a pile of n_rec records whose
    windows are wider than the 64-entry hit mask: P pairs in the block, cut into min(64, ceil(P / 32768)) slices (2, ~10,
    the cap of 64).  How many slices phase 0 listed stays on the device: the oracle comparison is the check.  Then again
    with chunk_ranges splitting the batch, so that the blocks and their slice lists restart per chunk."""
    rng = np.random.default_rng(n_rec)
    text = "\n".join(pile(rng, "U", n_rec, 10000, 10000 + n_rec * 4, ["Q%d" % i for i in range(16)], min_ops=2, max_ops=8)) + "\n"
    g, c = build_index(str(tmp_path), text, bidirectional=False)
    fused_options(g)
    U = g.seq_id("U")
    hi = 10000 + n_rec * 4
    ranges = [(U, int(rng.integers(5000, 10000)), int(rng.integers(hi, hi + 4000))) for _ in range(n_ranges)]  # (each hits every record)
    st, _, _ = g.query_batch_stats(ranges, impg_amd.make_params(), counts=False, checksums=False)
    P = int(st.pairs)
    assert P == n_rec * n_ranges and P > ENT_SLICE_PAIRS and P >= 32 * g.num_entries()
    assert min(ENT_MAX_SLICES, -(-P // ENT_SLICE_PAIRS)) == slices, P
    cache = {}
    forms = ("stats", "attributed") if n_rec < 5000 else ("stats",)
    check_forms(g, c, ranges, {}, cache=cache, forms=forms, expect=dict(stats=ENT_SLOTS, attributed=ENT_QS), tag=(n_rec, P))
    if n_rec == 5000:  # (the rows of the 64-slice block, attributed, on a quarter of the block)
        check_forms(g, c, ranges[:128], {}, cache=cache, forms=("attributed",), expect=dict(attributed=ENT_QS), tag=(n_rec, "quarter"))
    g.set_option("chunk_ranges", 150)
    check_forms(g, c, ranges, {}, cache=cache, forms=("stats",), expect=dict(stats=ENT_SLOTS), tag=(n_rec, P, "chunks"))
    g.set_option("chunk_ranges", 0)


# ---- d. the edge fixtures through every arm, one child process per switch -----------------------------------------------------
def test_edge_fixtures_through_every_arm():
    """tests/proj_worker.py, a fresh process per setting of the projection switches (each is read once per process): the
    edge fixtures of test_gpu_parity.py and random_paf's weird / inconsistent / long records, every form against the oracle,
    and the kernel each setting forces asserted to have run.  A child that dies on a signal or times out ends the test."""
    for setting, (var, val) in SETTINGS.items():
        env = dict(os.environ)
        env[var] = val
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "proj_worker.py"), setting], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=240)
        out = p.stdout[-4000:] + p.stderr[-4000:]
        if p.returncode < 0:
            pytest.fail("proj_worker %s died on signal %s; no further child started:\n%s" % (setting, signal.Signals(-p.returncode).name, out))
        assert p.returncode == 0, "proj_worker %s failed:\n%s" % (setting, out)
        assert "proj_worker %s ok" % setting in p.stdout, out


# ---- e. ranges already in HBM ---------------------------------------------------------------------------------------------------
def test_device_resident_ranges(tmp_path, threshold_index):
    """query_batch_stats / query_batch_device with device_ptr= (the timed path of bench.py): the same counts, checksums,
    projected and rows of every layout as the host ranges, and the oracle's."""
    import torch
    for name in ("threshold", "random"):
        if name == "threshold":
            g, c = threshold_index
            ranges = covering(g, "T", 160, 9000, 15000, 160) + covering(g, "T", 40, 11000, 12000, 3)
        else:
            text, _ = random_paf(71, 900, weird=True)
            g, c = build_index(str(tmp_path), text)
            ranges = random_ranges(72, 700, 6, 20000, max_len=5000)
        fused_options(g)
        r = impg_amd.GpuImpg._ranges(ranges)
        d = torch.from_numpy(r.view(np.uint8)).to("cuda:0")
        cache = {}
        for kw in ({}, M1, dict(M2, max_depth=3), dict(min_identity=0.8)):
            forms = ("stats", "attributed", "ordered", "slots")
            host = check_forms(g, c, ranges, kw, forms=forms, cache=cache, tag=(name, "host"))
            on_dev = check_forms(g, c, ranges, kw, forms=forms, cache=cache, device_ranges=d, tag=(name, "device"))
            assert on_dev == host, (name, kw, host, on_dev)  # (the same kernels, the same pairs)
            for chunk in (0, 97):
                g.set_option("chunk_ranges", chunk)
                a = g.query_batch_stats(ranges, impg_amd.make_params(**kw))
                b = g.query_batch_stats(None, impg_amd.make_params(**kw), device_ptr=d.data_ptr(), n=len(ranges))
                assert a[0].projected == b[0].projected and (a[1] == b[1]).all() and (a[2] == b[2]).all(), (name, kw, chunk)
            g.set_option("chunk_ranges", 0)
        del d
        torch.cuda.synchronize()


@pytest.mark.parametrize("bad", [(500, 500), (700, 400)])
def test_device_ranges_start_not_below_end_are_refused(threshold_index, bad):
    """A range with start >= end is refused (IMPG_E_INVALID) from HBM as from the host, in every form, before any row is
    returned; the engine answers the next batch normally."""
    import torch
    g, c = threshold_index
    fused_options(g)
    T = g.seq_id("T")
    good = covering(g, "T", 200, 9000, 15000, 9)
    for at in (0, 150):  # (in the first block, and behind a chunk boundary)
        ranges = list(good)
        ranges.insert(at, (T,) + bad)
        r = impg_amd.GpuImpg._ranges(ranges)
        d = torch.from_numpy(r.view(np.uint8)).to("cuda:0")
        for chunk in (0, 100):
            g.set_option("chunk_ranges", chunk)
            with pytest.raises(impg_amd.ImpgGpuError) as e:
                g.query_batch_stats(ranges, impg_amd.make_params())
            assert e.value.code == impg_amd.IMPG_E_INVALID
            calls = [lambda: g.query_batch_stats(None, impg_amd.make_params(), device_ptr=d.data_ptr(), n=len(ranges))]
            for layout in (impg_amd._lib.ROWS_ATTRIBUTED, impg_amd._lib.ROWS_ORDERED, impg_amd._lib.ROWS_ORDERED_SLOTS):
                calls.append(lambda layout=layout: g.query_batch_device(None, impg_amd.make_params(), device_ptr=d.data_ptr(), n=len(ranges), layout=layout))
            for call in calls:
                with pytest.raises(impg_amd.ImpgGpuError) as e:
                    call()
                assert e.value.code == impg_amd.IMPG_E_INVALID, e.value
        g.set_option("chunk_ranges", 0)
        del d
    check_forms(g, c, good, {}, forms=("stats", "slots"), expect=dict(stats=ENT_SLOTS))
