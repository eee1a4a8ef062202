"""bench.py --dump-outputs, on the CPU: the library's device arrays stood in for by host buffers, torch on the CPU.  The dump
must attribute every live slot to its range through source[] -> frontier[] exactly as the suite's _device_rows_by_range
does, never read a hole's source, keep the ordered layout's emission order, and hold every integer exactly."""
import os
import types

import numpy as np
import torch

import bench


class FakeDevice:
    """Host buffers of int32 words at made-up addresses; bench._device_words reads them, inside their bounds only."""

    def __init__(self):
        self.mem, self.next = {}, 1 << 20

    def alloc(self, a):
        w = np.ascontiguousarray(a, dtype=np.int32).ravel()
        base, self.next = self.next, self.next + (w.size + 64) * 4
        self.mem[base] = w
        return base

    def words(self, ptr, shape, dev):
        for base, w in self.mem.items():
            if base <= ptr < base + w.size * 4:
                off, n = (ptr - base) // 4, int(np.prod(shape))
                assert off + n <= w.size, "read past the end of a device array"
                return torch.from_numpy(w[off:off + n].reshape(shape).copy())
        raise AssertionError("unknown device address")


class FakeRows:
    def __init__(self, parts, cnt=None, ck=None):
        self._parts, self.cnt, self.ck, self.freed = parts, cnt, ck, False
        self.projected = int(cnt.sum()) if cnt is not None else 0

    def parts(self):
        return self._parts

    def check(self):
        return self.cnt.copy(), self.ck.copy()

    def free(self):
        self.freed = True


def _dump(tmp_path, monkeypatch, fake, form, dr, n):
    monkeypatch.setattr(bench, "_device_words", fake.words)
    st = types.SimpleNamespace(projected=dr.projected)
    info = bench.dump_outputs(str(tmp_path), form, {"rows": dr}, [st], np.zeros(n), "cpu", None, 1, 0)
    assert dr.freed
    return info, {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}


def test_dump_attributed_rows(tmp_path, monkeypatch):
    rng, fake, n = np.random.default_rng(7), FakeDevice(), 500
    parts, want = [], [[] for _ in range(n)]
    for first, nr, ns, nf, stride in [(0, 300, 2000, 300, 1), (0, 300, 50000, 700, 2), (300, 200, 30000, 400, 2), (300, 200, 0, 0, 2)]:
        fr = np.column_stack([rng.integers(0, 50, nf), np.zeros(nf), np.zeros(nf), rng.integers(0, nr, nf)]).astype(np.int32)
        qid = rng.integers(0, 50, ns).astype(np.int32)
        src = rng.integers(0, max(nf, 1), ns).astype(np.int32)
        co = rng.integers(0, 5_000_000, (ns, 4)).astype(np.int32)
        hole = rng.random(ns) < 0.1
        qid[hole], src[hole] = -1, 10 ** 6  # a hole's source is garbage: never an index
        p = types.SimpleNamespace(first_range=first, n_ranges=nr, n_frontier=nf, slot_stride=stride, n_slots=ns,
                                  coords=fake.alloc(co), frontier=fake.alloc(fr))
        if stride == 2:  # query_id and source side by side
            p.query_id = fake.alloc(np.column_stack([qid, src]))
            p.source = p.query_id + 4
        else:
            p.query_id, p.source = fake.alloc(qid), fake.alloc(src)
        parts.append(p)
        for s in np.flatnonzero(~hole):
            f = fr[src[s]]
            want[first + f[3]].append((first + int(f[3]), int(qid[s]), int(co[s, 0]), int(co[s, 1]), int(f[0]), int(co[s, 2]), int(co[s, 3])))
    cnt = np.array([len(w) for w in want], dtype=np.uint64)
    ck = rng.integers(0, 2 ** 63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    info, got = _dump(tmp_path, monkeypatch, fake, "rows", FakeRows(parts, cnt, ck), n)
    assert sorted(got) == ["projected", "range_checksums", "range_counts", "sample_ranges", "sample_rows"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    sample = got["sample_ranges"].astype(np.int64)
    assert len(sample) == bench.DUMP_SAMPLE_RANGES and (np.diff(sample) > 0).all()
    assert [tuple(int(x) for x in r) for r in got["sample_rows"]] == sorted(r for i in sample for r in want[i])
    assert (got["range_counts"] == cnt).all()
    hi, lo = got["range_checksums"].T.astype(np.uint64)
    assert ((hi << np.uint64(32)) | lo == ck).all()
    chk = {"status": "ok", "expected": None}
    bench.self_check_dumped(info, chk)
    assert chk["status"] == "ok" and chk["dumped_rows"]["stray_slots"] == 0


def test_dump_ordered_rows(tmp_path, monkeypatch):
    rng, fake, n = np.random.default_rng(8), FakeDevice(), 500
    parts, want, slots = [], [[] for _ in range(n)], np.zeros(n)
    for first, nr in ((0, 300), (300, 200)):
        per = rng.integers(0, 40, nr)
        off = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
        iv = rng.integers(0, 5_000_000, (int(off[-1]), 6)).astype(np.int32)
        iv[rng.random(len(iv)) < 0.1, 0] = -1  # hole rows
        slots[first:first + nr] = per
        for r in range(nr):
            want[first + r] = [(first + r,) + tuple(int(x) for x in v) for v in iv[off[r]:off[r + 1]] if v[0] != -1]
        parts.append(types.SimpleNamespace(first_range=first, n_ranges=nr, n_slots=len(iv), rows=fake.alloc(iv), offsets=fake.alloc(off)))
    info, got = _dump(tmp_path, monkeypatch, fake, "ordered", FakeRows(parts), n)
    sample = got["sample_ranges"].astype(np.int64)
    assert [tuple(int(x) for x in r) for r in got["sample_rows"]] == [r for i in sample for r in want[i]]  # emission order kept
    assert (got["range_slots"] == slots).all()
    assert info["_rows_check"]["bad_offsets"] == 0


def test_dump_float_exact():
    assert bench._exact_float([0, (1 << 24) - 1]).dtype == np.float32
    big = bench._exact_float([-(1 << 24), 5])
    assert big.dtype == np.float64 and int(big[0]) == -(1 << 24)
