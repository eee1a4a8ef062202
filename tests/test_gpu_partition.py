"""`impg partition` on the GPU: the device-resident region algebra against the host twin and the sequential
restatement (tests/partition_ref.py), the session end to end against the restatement's partitions.bed, what stays in
HBM, and what is refused."""
import os

import numpy as np
import pytest

import impg_amd
from impg_amd import _lib
from oracle import oracle as o
from tests import partition_ref as pr

pytestmark = pytest.mark.gpu


def test_device_algebra_equals_host_twin_and_reference():
    rng = np.random.default_rng(5)
    windows = pr.scripted_windows() + pr.random_windows(rng, pr.LENS, 40 - len(pr.scripted_windows()))
    windows += [[(2, 30900, 30950)], []]  # exactly one row; no row at all
    ref = pr.Ref(pr.LENS)
    dev = impg_amd.Regions(pr.LENS, on_host=False)
    host = impg_amd.Regions(pr.LENS, on_host=True)
    for k, rows in enumerate(windows):
        a = pr.rows_array(rows)
        want = ref.apply(rows, 100, 300, 200)
        assert host.apply(a, 100, 300, 200) == want, k
        assert dev.apply(a, 100, 300, 200) == want, k
        assert dev.get("masked") == ref.masked.table(), k
        assert dev.get("missing") == ref.missing.table(), k
        for mode in ("longest", "total"):
            assert dev.select(mode, 5000) == ref.select(mode, 5000), (k, mode)
    assert ref.count["extensions"] > 0 and ref.count["splits"] > 0 and ref.count["empty_windows"] > 0


def test_device_algebra_many_rows():
    """100 000 rows on 3 sequences: several workgroups in every sort, scan and compaction; host twin as the yardstick,
    the restatement on a thinned prefix."""
    lens = [3_000_000, 2_000_001, 1_234_567]
    rng = np.random.default_rng(11)
    dev = impg_amd.Regions(lens, on_host=False)
    host = impg_amd.Regions(lens, on_host=True)
    ref = pr.Ref(lens)
    first = pr.random_windows(rng, lens, 1, max_rows=200)[0]
    assert dev.apply(pr.rows_array(first), 10, 50, 40) == ref.apply(first, 10, 50, 40) == host.apply(pr.rows_array(first), 10, 50, 40)
    n = 100_000
    s = rng.integers(0, 3, n)
    ln = rng.integers(1, 40, n)
    a = (rng.random(n) * (np.array(lens)[s] - ln)).astype(np.int64)
    rev = rng.random(n) < 0.3
    rows = np.zeros(n, dtype=_lib.INTERVAL_DTYPE)
    rows["query_id"] = s
    rows["q_first"] = np.where(rev, a + ln, a)
    rows["q_last"] = np.where(rev, a, a + ln)
    for d in (10, 0):  # the second pass meets the first one's mask: every interval is split or swallowed
        want = host.apply(rows, d, 50, 40)
        got = dev.apply(rows, d, 50, 40)
        assert len(want) > (20_000 if d else 0)
        assert got == want
        assert dev.get("masked") == host.get("masked")
        assert dev.get("missing") == host.get("missing")
        rows["q_first"] += 15
        rows["q_last"] += 15
        assert dev.select("longest", 10_000_000) == host.select("longest", 10_000_000)
        assert dev.select("total", 10_000_000) == host.select("total", 10_000_000)


SEED, N_REC = int(os.environ.get("PARTITION_SEED", 3)), 2000
SHAPE = dict(n_seq=20, seq_len=200_000, target_span=10_000, n_blocks=100)
RUN = dict(window_size=20_000, merge_distance=1000)


@pytest.fixture(scope="module")
def paf(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("partition") / "synth.paf")
    impg_amd.synth_paf_text(path, SEED, N_REC, **SHAPE)
    return path


@pytest.fixture(scope="module")
def cpu(paf):
    return o.OracleIndex(paf_paths=[paf], preparse=True)


@pytest.fixture(scope="module")
def gpu(paf):
    return impg_amd.GpuImpg.from_paf(paf)


@pytest.fixture(scope="module")
def reference_run(cpu):
    ref, parts, text = pr.partition(cpu, RUN["window_size"], RUN["merge_distance"], max_depth=2)
    # the run must reach the cases it is about before the engine is looked at
    # (no window of a `longest` run can come back empty: it is cut from the missing set, so its own self interval
    # survives the mask; the windows without a partition are asserted in the starting-list run below)
    assert len(parts) >= 20 and ref.count["extensions"] >= 1
    assert ref.count["splits"] >= 1 and ref.count["rehomed"] >= 1, ref.count
    return ref, parts, text


def run_session(gpu, params, **kw):
    s = gpu.partition_session(RUN["window_size"], RUN["merge_distance"], params, **kw)
    try:
        text, n = s.run_text()
        reg = s.regions()
        counters = {k: s.counter(k) for k in ("windows", "partitions", "mask_uploads", "rows_to_host", "walk_windows", "step_launches")}
        return text, n, reg.get("masked"), reg.get("missing"), counters
    finally:
        s.close()


def test_end_to_end_bfs_and_residency(gpu, reference_run):
    ref, parts, want = reference_run
    p = impg_amd.make_params(transitive=True, max_depth=2)
    text, n, masked, missing, c = run_session(gpu, p)
    assert text == want
    assert masked == ref.masked.table() and missing == ref.missing.table()
    assert c["mask_uploads"] == 0 and c["rows_to_host"] == 0 and c["walk_windows"] > 0 and c["step_launches"] > 0
    assert c["windows"] - c["partitions"] == ref.count["empty_windows"]
    text_h, _, masked_h, missing_h, ch = run_session(gpu, p, state_on_host=True)
    assert text_h == want and masked_h == masked and missing_h == missing
    assert ch["mask_uploads"] > 0 and ch["rows_to_host"] > 0


@pytest.mark.parametrize("case", ["dfs", "total", "starting"])
def test_end_to_end_variants(gpu, cpu, case):
    qkw = dict(max_depth=2, dfs=case == "dfs")
    kw = {}
    rkw = {}
    if case == "total":
        kw["selection_mode"] = rkw["selection_mode"] = "total"
    if case == "starting":
        names = [cpu.seq_name(3), cpu.seq_name(3)]  # the second pass over a sequence finds it masked: windows without a partition
        kw["starting_sequences"] = names
        rkw["starting"] = [cpu.seq_id(n) for n in names]
    ref, parts, want = pr.partition(cpu, RUN["window_size"], RUN["merge_distance"], **rkw, **qkw)
    assert len(parts) >= 5
    if case == "starting":
        assert ref.count["empty_windows"] >= 1, ref.count
    text, n, masked, missing, c = run_session(gpu, impg_amd.make_params(transitive=True, **qkw), **kw)
    assert text == want
    assert masked == ref.masked.table() and missing == ref.missing.table()
    assert c["mask_uploads"] == 0 and c["rows_to_host"] == 0


def test_generator_yields_partitions_before_rehoming(gpu, cpu):
    ref, parts, _ = pr.partition(cpu, RUN["window_size"], RUN["merge_distance"], rehome=False, max_depth=2, max_windows=12)
    got = []
    for num, rows in gpu.partition(RUN["window_size"], RUN["merge_distance"], impg_amd.make_params(transitive=True, max_depth=2)):
        got.append((num, rows))
        if len(got) == len(parts):
            break
    assert got == parts


def test_window_larger_than_the_callers_buffer(gpu, cpu):
    ref, parts, _ = pr.partition(cpu, RUN["window_size"], RUN["merge_distance"], rehome=False, max_depth=2, max_windows=3)
    assert max(len(rows) for _, rows in parts) > 2
    for host in (False, True):
        s = gpu.partition_session(RUN["window_size"], RUN["merge_distance"], impg_amd.make_params(transitive=True, max_depth=2),
                                  state_on_host=host)
        try:
            got = [s.window(*w, cap=2) for w in s.next_windows()[:1]]  # two rows fit; the rest is fetched from the session
            assert got[0] == parts[0][1]
            assert s.regions().get("masked")[parts[0][1][0][0]] != []
        finally:
            s.close()


def test_traffic_counters_are_read_where_the_copies_happen(gpu):
    """The session's counters are deltas of the index's own, bumped at the copy sites: a masked query with a host mask
    through the same handle moves them, a device-state window does not."""
    p = impg_amd.make_params(transitive=True, max_depth=2)
    s = gpu.partition_session(RUN["window_size"], RUN["merge_distance"], p)
    try:
        w = s.next_windows()[0]
        assert s.window(*w)
        assert s.counter("mask_uploads") == 0 and s.counter("rows_to_host") == 0
    finally:
        s.close()
    h = gpu.partition_session(RUN["window_size"], RUN["merge_distance"], p, state_on_host=True)
    try:
        w = h.next_windows()[0]
        assert h.window(*w)
        assert h.counter("mask_uploads") == 3      # offsets and the two length arrays: the mask holds no range yet
        first = h.counter("rows_to_host")
        assert first > 0
        w = h.next_windows()[0]
        h.window(*w)
        assert h.counter("mask_uploads") == 7      # ... and now its ranges as well
        assert h.counter("rows_to_host") > first
    finally:
        h.close()


def test_refusals(gpu, paf):
    ok = impg_amd.make_params(transitive=True, max_depth=2)

    def code(params, **kw):
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            gpu.partition_session(kw.pop("w", 20_000), kw.pop("d", 1000), params, **kw)
        return e.value.code

    assert code(ok, d=-1) == impg_amd.IMPG_E_INVALID
    assert code(impg_amd.make_params(transitive=True, store_cigar=True)) == impg_amd.IMPG_E_INVALID
    assert code(impg_amd.make_params(transitive=False)) == impg_amd.IMPG_E_INVALID
    assert code(impg_amd.make_params(transitive=True, min_output_length=10)) == impg_amd.IMPG_E_INVALID
    multi = impg_amd.GpuImpg.from_paf(paf, devices=[0, 0])
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        multi.partition_session(20_000, 1000, ok)
    assert e.value.code == impg_amd.IMPG_E_UNSUPPORTED


def test_create_does_not_wait_for_an_engine(gpu):
    ok = impg_amd.make_params(transitive=True, max_depth=2)
    held = []
    try:
        for _ in range(4):  # every engine of the handle pinned by a device-rows handle
            held.append(gpu.query_batch_device([(0, 0, 1000)], impg_amd.make_params()))
        with pytest.raises(impg_amd.ImpgGpuError) as e:
            gpu.partition_session(20_000, 1000, ok)
        assert e.value.code == impg_amd.IMPG_E_UNSUPPORTED
        s = gpu.partition_session(20_000, 1000, ok, state_on_host=True)  # holds no engine: may be made
        s.close()
    finally:
        for h in held:
            h.free()
    s = gpu.partition_session(20_000, 1000, ok)
    s.close()


def test_cli(paf, cpu, reference_run, tmp_path):
    import subprocess
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "impg-gpu")
    _, _, want = reference_run
    base = [exe, "partition", "-a", paf, "-w", "20000", "-d", "1000", "-m", "2"]
    one = tmp_path / "one"
    subprocess.run(base + ["--output-folder", str(one)], check=True, timeout=120)
    assert (one / "partitions.bed").read_text() == want
    _, parts, _ = pr.partition(cpu, RUN["window_size"], RUN["merge_distance"], rehome=False, max_depth=2)
    many = tmp_path / "many"
    subprocess.run(base + ["--output-folder", str(many), "--separate-files"], check=True, timeout=120)
    names = [cpu.seq_name(s) for s in range(cpu.num_seqs())]
    assert sorted(os.listdir(many)) == sorted("partition%d.bed" % k for k, _ in parts)
    for k, ivs in parts:
        assert (many / ("partition%d.bed" % k)).read_text() == "".join("%s\t%d\t%d\n" % (names[s], a, b) for s, a, b in ivs)
    assert subprocess.run(base + ["-o", "gfa"], timeout=60).returncode == 2
    assert subprocess.run([exe, "partition", "-a", paf, "-w", "0", "-d", "5"], timeout=60).returncode != 0
    assert subprocess.run([exe, "partition", "-a", paf, "-w", "20000"], timeout=60).returncode != 0


def test_real_data():
    """One of the stored reference PAFs (sequences of a few hundred bases: a window of 25 gives 11 partitions)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_paf", "short_floor.paf")
    c = o.OracleIndex(paf_paths=[path], preparse=True)
    qkw = dict(max_depth=2, min_transitive_len=5, min_distance_between_ranges=2)
    ref, parts, want = pr.partition(c, 25, 3, 8, 6, **qkw)
    assert len(parts) >= 5
    g = impg_amd.GpuImpg.from_paf(path)
    for host in (False, True):
        s = g.partition_session(25, 3, impg_amd.make_params(transitive=True, **qkw), min_missing_size=8, min_boundary_distance=6,
                                state_on_host=host)
        try:
            assert s.run_text()[0] == want
            assert s.regions().get("masked") == ref.masked.table() and s.regions().get("missing") == ref.missing.table()
        finally:
            s.close()
