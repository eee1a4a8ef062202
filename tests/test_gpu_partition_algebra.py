"""The device partition algebra (impg_amd/csrc/partition_device.hip) on small, collision-dense universes and at the
edges of its blocks and tables: after every window the device object and the host twin against the sequential
restatement (tests/partition_ref.py) -- output rows, both tables, `longest` and `total` -- all of it exact.  Every input
comes from partition_ref.py's generators; tests/test_partition_cpu.py proves the same inputs on the host twin."""
import numpy as np
import pytest
import torch  # (brings a HIP runtime of its own: loaded before libimpg_gpu.so initialises the system's, or it finds no device)

import impg_amd
from tests import partition_ref as pr

pytestmark = pytest.mark.gpu

DENSE_SEEDS = range(150)


def both(lens):
    return impg_amd.Regions(lens, on_host=False), impg_amd.Regions(lens, on_host=True)


@pytest.mark.parametrize("variant", list(pr.DENSE_VARIANTS))
def test_dense_universes(variant):
    cases, reached = pr.dense_reference(DENSE_SEEDS, **pr.DENSE_VARIANTS[variant])
    # the seeds reach what the test is about: asserted from the restatement alone, before the device is looked at
    want = pr.DENSE_REACH + ([pr.ZERO_LEN_REACH] if variant == "zero_len" else [])
    assert [c for c in want if c not in reached] == []
    for seed, lens, w, steps in cases:
        for reg in both(lens):
            try:
                pr.replay(reg, steps, w)
            except AssertionError as e:
                raise AssertionError("seed %d, lens %r: %s" % (seed, lens, e)) from e
            reg.close()


@pytest.mark.parametrize("n_seq", [1, 2, 255, 256, 257, 1024])
def test_sequence_counts(n_seq):
    """Most sequences untouched, a few of length 0: the table kernels' per-sequence offsets at a workgroup edge."""
    lens, params, windows = pr.sparse_case(n_seq)
    steps = pr.ref_steps(pr.Ref(lens), windows, params, max(lens))
    for reg in both(lens):
        pr.replay(reg, steps, max(lens))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_row_counts(n):
    """n rows that stay n intervals: every per-item kernel with its last workgroup partly full, on a fresh object
    (n_old = 0) and on the warm state."""
    lens, windows = pr.row_count_case(n)
    ref = pr.Ref(lens)
    steps = [st for rows, params in windows for st in pr.ref_steps(ref, [rows], params, lens[0])]
    assert [len(st[2]) for st in steps] == [n, n, n, 0] and ref.count["extensions"] == 2 * n - min(n, 2)
    for reg in both(lens):
        pr.replay(reg, steps, lens[0])


def test_piece_counts():
    """Windows that leave exactly 0, 1 and 2 pieces (the second sort runs from 2 on), fresh and warm."""
    lens, params, windows = pr.piece_count_case()
    steps = pr.ref_steps(pr.Ref(lens), [rows for rows, _ in windows], params, 100)
    assert [len(st[2]) for st in steps] == [pieces for _, pieces in windows]
    assert {pieces for _, pieces in windows} >= {0, 1, 2}
    for reg in both(lens):
        pr.replay(reg, steps, 100)


def test_length_above_int32_is_clamped():
    given, kept, params, windows = pr.clamp_case()
    steps = pr.ref_steps(pr.Ref(kept), windows, params, pr.I32_MAX)
    for reg in both(given):
        assert reg.get("missing")[0] == [(0, pr.I32_MAX)]
        assert reg.select("longest", pr.I32_MAX) == [(0, 0, pr.I32_MAX)]
        pr.replay(reg, steps, pr.I32_MAX)


# ---- selection ties on the device ---------------------------------------------------------------------------------------
NAMES = ["A#1#chr1", "A#1#chr2", "A#2#chr1", "B#1#chr1", "B#1#chr2", "C#1#chr1"]
MODES = ("longest", "total", "sample", "haplotype", "haplotype,#", "sample,#")


def test_select_modes_on_the_device():
    """test_partition_cpu.py::test_select_modes' two scripts and its literal expectations, on the device state."""
    lens = [30000, 30000, 45000, 40000, 15000, 10000]
    ref = pr.Ref(lens)
    reg = impg_amd.Regions(lens, on_host=False)
    for rows in [[(0, 10000, 20000)], [(1, 5000, 15000)], [(2, 0, 45000)], [(3, 0, 30000)]]:
        assert reg.apply(pr.rows_array(rows), 0, 0, 0) == ref.apply(rows, 0, 0, 0)
    for mode in MODES:
        for w in (4000, 7000, 100000):
            assert reg.select(mode, w, NAMES) == ref.select(mode, w, NAMES), (mode, w)
    assert reg.select("longest", 100000) == [(4, 0, 15000)]  # 15000 on 1 and on 4: the higher id wins
    assert reg.select("total", 100000) == [(1, 0, 30000)]    # 20000 missing bases on 0 and on 1: the higher id wins
    assert reg.select("sample", 100000, NAMES) == [(0, 0, 30000), (1, 0, 30000)]
    assert reg.select("haplotype,#", 100000, NAMES) == [(0, 0, 30000), (1, 0, 30000)]
    for rows in [[(4, 0, 15000)], [(3, 30000, 40000)], [(5, 0, 10000)], [(1, 15000, 20000)]]:
        assert reg.apply(pr.rows_array(rows), 0, 0, 0) == ref.apply(rows, 0, 0, 0)
    for mode in MODES:
        for w in (4000, 7000, 100000):
            assert reg.select(mode, w, NAMES) == ref.select(mode, w, NAMES), (mode, w)
    assert reg.select("longest", 100000) == [(1, 20000, 30000)]  # the later range of the higher sequence
    assert reg.select("longest", 4000) == [(1, 20000, 24000), (1, 24000, 30000)]  # the tail window joins its predecessor
    with pytest.raises(ValueError):
        reg.select("largest", 10)


def test_dense_ties():
    lens, params, windows = pr.tie_case()
    modes = ("longest", "total", "sample", "haplotype")
    for w in (1000, 300):
        steps = pr.ref_steps(pr.Ref(lens), windows, params, w, pr.TIE_NAMES, modes)
        for reg in both(lens):
            pr.replay(reg, steps, w, pr.TIE_NAMES)


# ---- a refused call leaves the state as it was --------------------------------------------------------------------------
def agrees(reg, ref):
    masked, missing = pr.ref_tables(ref)
    assert reg.get("masked") == masked and reg.get("missing") == missing
    for mode in ("longest", "total", "sample", "haplotype"):
        assert reg.select(mode, 1000, pr.REFUSAL_NAMES) == ref.select(mode, 1000, pr.REFUSAL_NAMES), mode


@pytest.mark.parametrize("fresh", [False, True], ids=["warm", "fresh"])
@pytest.mark.parametrize("bad", [(3, 0, 10), (1, -5, 10), (1, 10, -5)], ids=["seq_id", "negative_first", "negative_last"])
@pytest.mark.parametrize("where", ["host_rows", "device_rows"])
def test_refusal_leaves_the_state_as_it_was(where, bad, fresh):
    """host_rows: impg_gpu_regions_apply refuses before anything runs.  device_rows: the rows lie in HBM as a session's
    do, nothing reads them on the host, and the refusal is DeviceRegions::apply's own, made after every kernel of the
    window has run."""
    lens, params, before, valid, after = pr.refusal_case(fresh)
    ref = pr.Ref(lens)
    dev, host = both(lens)
    for rows in before:
        want = ref.apply(rows, *params)
        assert dev.apply(pr.rows_array(rows), *params) == want == host.apply(pr.rows_array(rows), *params)
    moved = pr.Ref(lens)  # the valid rows alone would change every answer that is read from the sums
    for rows in before + [valid]:
        moved.apply(rows, *params)
    for mode in ("total", "haplotype"):
        assert moved.select(mode, 1000, pr.REFUSAL_NAMES) != ref.select(mode, 1000, pr.REFUSAL_NAMES)
    a = pr.rows_array(valid[:1] + [(0, 0, 0)] + valid[1:])
    a[1]["query_id"], a[1]["q_first"], a[1]["q_last"] = bad
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        if where == "host_rows":
            dev.apply(a, *params)
        else:
            d = torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            dev.apply(None, *params, device_ptr=d.data_ptr(), n=a.size)
    assert e.value.code == impg_amd.IMPG_E_INVALID
    with pytest.raises(impg_amd.ImpgGpuError) as e:
        host.apply(a, *params)
    assert e.value.code == impg_amd.IMPG_E_INVALID
    agrees(dev, ref)
    agrees(host, ref)
    want = ref.apply(after, *params)
    if where == "device_rows":  # the accepted call through the same entry
        d = torch.from_numpy(np.frombuffer(pr.rows_array(after).tobytes(), dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        assert dev.apply(None, *params, device_ptr=d.data_ptr(), n=len(after)) == want
    else:
        assert dev.apply(pr.rows_array(after), *params) == want
    assert host.apply(pr.rows_array(after), *params) == want
    agrees(dev, ref)
    agrees(host, ref)
