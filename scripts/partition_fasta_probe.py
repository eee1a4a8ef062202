#!/usr/bin/env python3
"""Per-window and per-byte cost of `impg partition -o fasta` beside the BED session.  Writes profiles/partition_fasta_probe.json.

Workload: impg_synth_paf_text, 10^6 records over the default sequence table (200 x 5 Mb), a store of random bases of
the same size; -w 100000 -d 10000 -m 3, BFS, longest; the first --windows windows of a fresh session, every leg run once
to warm up and then --repeats times, the median run reported with all of them beside it.  Legs:
  bed            session.window per window (query + update): the BED session's window, which this route must not change
  fasta_device   session.window_fasta to a file descriptor, state in HBM
  fasta_host     the same with state_on_host
  caller_loop    session.window rows + impg_amd.partition_fasta_text on the host + the write
  per_window     fasta_device with IMPG_PARTITION_TEXT_STREAM_PER_WINDOW=1: the stream allocated anew for every window
  piece_timing   fasta_device under IMPG_FASTA_PIECE_TIMING: every piece's write kernel and a plain D2H copy of the same
                 bytes between events (one run each for the byte and the packed store; it adds a copy, so its wall time
                 is not a leg)
Derived: ms per window and ns per text byte; kernel_over_copy = sum of kernel ms / sum of copy ms; outside_share = the
share of a FASTA window that is neither the BED window (query + update) nor the pieces' kernel and copy time, for the
session-lived stream and for the per-window one."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import impg_amd  # noqa: E402

W, D, DEPTH = 100_000, 10_000, 3
ALPHABET = np.frombuffer(b"ACGT", dtype=np.uint8)


def windows_of(s, n_windows):
    done = 0
    while done < n_windows:
        ws = s.next_windows()
        if not ws:
            return
        for w in ws[:n_windows - done]:
            yield w
            done += 1


def run(g, n_windows, kind, fd, store=None, names=None):
    s = g.partition_session(W, D, impg_amd.make_params(transitive=True, max_depth=DEPTH), state_on_host=kind == "fasta_host")
    n = text = 0
    try:
        t0 = time.perf_counter()
        for w in windows_of(s, n_windows):
            if kind == "bed":
                s.window(*w)
            elif kind == "caller_loop":
                rows = s.window(*w)
                if rows:
                    t = impg_amd.partition_fasta_text(store, names, rows)
                    os.write(fd, t)
                    text += len(t)
            else:
                before = os.fstat(fd).st_size
                s.window_fasta(*w, fd=fd)
                text += os.fstat(fd).st_size - before
            n += 1
        wall = time.perf_counter() - t0
        return dict(wall_s=wall, windows=n, text_bytes=text, text_buffer_allocs=s.counter("text_buffer_allocs"),
                    text_table_uploads=s.counter("text_table_uploads"))
    finally:
        s.close()
        os.ftruncate(fd, 0)
        os.lseek(fd, 0, os.SEEK_SET)


def leg(g, n_windows, kind, fd, repeats, **kw):
    run(g, n_windows, kind, fd, **kw)  # warm-up: engines, slabs, scratch, the pinned pool
    runs = [run(g, n_windows, kind, fd, **kw) for _ in range(repeats)]
    med = dict(sorted(runs, key=lambda r: r["wall_s"])[len(runs) // 2])
    med["wall_s_all"] = [r["wall_s"] for r in runs]
    med["ms_per_window"] = med["wall_s"] * 1e3 / max(1, med["windows"])
    med["ms_per_window_all"] = [r["wall_s"] * 1e3 / max(1, r["windows"]) for r in runs]
    if med["text_bytes"]:
        med["ns_per_text_byte"] = med["wall_s"] * 1e9 / med["text_bytes"]
    return med


def piece_timing(g, n_windows, fd, path):
    open(path, "w").close()
    os.environ["IMPG_FASTA_PIECE_TIMING"] = path
    try:
        r = run(g, n_windows, "fasta_device", fd)
    finally:
        del os.environ["IMPG_FASTA_PIECE_TIMING"]
    rows = [line.split() for line in open(path)]
    kernel, copy = sum(float(x[1]) for x in rows), sum(float(x[2]) for x in rows)
    return dict(pieces=len(rows), bytes=sum(int(x[0]) for x in rows), kernel_ms=kernel, copy_ms=copy, kernel_over_copy=kernel / copy if copy else None,
                windows=r["windows"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=300)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bed-only", action="store_true", help="the BED leg alone (what a checkout without the FASTA route can run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition_fasta_probe.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "probe.paf")
        impg_amd.synth_paf_text(path, 42, a.records)
        g = impg_amd.GpuImpg.from_paf(path)
        fd = os.open(os.path.join(d, "text.fasta"), os.O_RDWR | os.O_CREAT, 0o666)
        res = dict(workload=dict(records=a.records, window=W, merge_distance=D, max_depth=DEPTH, selection="longest", windows=a.windows,
                                 repeats=a.repeats))
        res["bed"] = leg(g, a.windows, "bed", fd, a.repeats)
        if not a.bed_only:
            n = g.num_seqs()
            names = [g.seq_name(q) for q in range(n)]
            rng = np.random.default_rng(42)
            store = impg_amd.Sequences.from_arrays(names, [ALPHABET[rng.integers(0, 4, size=g.seq_len(q))].tobytes() for q in range(n)])
            res["workload"]["store_bases"] = sum(g.seq_len(q) for q in range(n))
            g.set_sequences(store, packed=False)
            for kind in ("fasta_device", "fasta_host"):
                res[kind] = leg(g, a.windows, kind, fd, a.repeats)
            res["caller_loop"] = leg(g, a.windows, "caller_loop", fd, a.repeats, store=store, names=names)
            os.environ["IMPG_PARTITION_TEXT_STREAM_PER_WINDOW"] = "1"
            try:
                res["per_window"] = leg(g, a.windows, "fasta_device", fd, a.repeats)
            finally:
                del os.environ["IMPG_PARTITION_TEXT_STREAM_PER_WINDOW"]
            res["piece_timing"] = piece_timing(g, a.windows, fd, os.path.join(d, "pieces.txt"))
            g.set_sequences(store, packed=True)
            res["piece_timing_packed"] = piece_timing(g, a.windows, fd, os.path.join(d, "pieces_packed.txt"))
            pieces_ms = (res["piece_timing"]["kernel_ms"] + res["piece_timing"]["copy_ms"]) / max(1, res["piece_timing"]["windows"])
            for kind in ("fasta_device", "per_window"):
                ms = res[kind]["ms_per_window"]
                res[kind]["outside_share"] = (ms - res["bed"]["ms_per_window"] - pieces_ms) / ms
        os.close(fd)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
