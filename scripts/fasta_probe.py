"""Device FASTA against its host twin on the headline index: impg_gpu_query_batch_fasta_fd (query, the query-axis sweep and
the records written on the device from the sequence store in HBM, the text to /dev/null as the command line writes it to
stdout) against query_batch + impg_gpu_results_fasta (rows across PCIe, sweep and text on host threads), in one process.

  python scripts/fasta_probe.py [--records 1000000] [--ranges 10000] [--out profiles/fasta_probe.json]

The index is the 1 M-record synthetic one (200 sequences of 5 Mb); the store holds 200 seeded random sequences of those
lengths; the batch is the 10 000-range `-x -m 2` batch at d = 0.  One warm-up, then three runs of the device route (median
and spread, with seconds3 {engine, rows + merge, text}); then one run under IMPG_FASTA_PIECE_TIMING: every piece's write
kernel between two events, and a copy of the same piece to a pinned buffer between two more -- the kernel is meant to hide
behind that copy.  The host twin runs twice on the ranges whose text fits --host-bytes (all of them if the whole text does),
the device route is timed on the same ranges, and both texts must be equal byte for byte.  The json is rewritten after every
stage, so a run that is cut short leaves what it measured.

  python scripts/fasta_probe.py --store bytes,packed --n-layout scattered,runs --out profiles/fasta_packed_probe.json

--store bytes|packed is the form the store takes in HBM (option "sequence_store_packed"), --n-layout scattered|runs where the
2 % of N lie: every one placed at random -- about one run per 50 bases, the packed form's bad case -- or the same number as
four long runs per sequence, as assemblies hold them.  The defaults are the run described above.  Given more than one
value (comma-separated), the probe measures every leg in one process on one index and one batch instead: the attach, the
store's counters, three runs of the device route, the pieces' kernel against their copies, and whether the legs of one
layout print the same bytes on the --host-bytes ranges."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import impg_amd  # noqa: E402
from impg_amd import _lib  # noqa: E402

FASTA_COUNTERS = ("fasta_rows", "fasta_records", "fasta_text_pieces", "fasta_text_bytes", "fasta_store_bytes", "fasta_store_packed",
                  "fasta_store_exception_runs")
N_SHARE = 0.02


def one_sequence(rng, seq_len, layout):
    """the sequence every store sequence is a rotation of: 2 % N, scattered or as four long runs"""
    if layout == "scattered":
        return np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, size=seq_len, p=[(1 - N_SHARE) / 4] * 4 + [N_SHARE])]
    one = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=seq_len)]
    run = int(seq_len * N_SHARE) // 4
    for k in range(4):
        at = seq_len * k // 4 + int(rng.integers(0, seq_len // 4 - run))
        one[at:at + run] = ord("N")
    return one


def piece_timing(device, ranges):
    """one run under IMPG_FASTA_PIECE_TIMING: every piece's write kernel against a copy of the same piece"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "pieces.txt")
        os.environ["IMPG_FASTA_PIECE_TIMING"] = path
        try:
            device(ranges)
        finally:
            del os.environ["IMPG_FASTA_PIECE_TIMING"]
        pieces = [dict(zip(("bytes", "kernel_ms", "copy_ms"), (int(a), float(b), float(c)))) for a, b, c in (ln.split() for ln in open(path))]
    kb, km, cm = (sum(x[k] for x in pieces) for k in ("bytes", "kernel_ms", "copy_ms"))
    return {"per_piece": pieces, "bytes": kb, "kernel_ms": km, "copy_ms": cm, "kernel_over_copy": km / cm if cm else None,
            "kernel_text_bytes_per_second": kb / (km * 1e-3) if km else None, "copy_bytes_per_second": kb / (cm * 1e-3) if cm else None}


def store_legs(args, g, n_seq, seq_len, ranges, p, d, stores, layouts):
    """every (layout, store form) leg on one index and one batch -> args.out"""
    import zlib
    out = {"index": {"records": args.records, "sequences": n_seq, "sequence_length": seq_len}, "ranges": args.ranges, "range_length": 5000,
           "leg": "-x -m 2", "merge_distance": d, "n_share": N_SHARE, "legs": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    null = os.open(os.devnull, os.O_WRONLY)

    def device(r):
        t0 = time.perf_counter()
        n, sec = g.query_batch_fasta(r, p, merge_distance=d, fd=null, timing=True)
        return time.perf_counter() - t0, sec, n

    for layout in layouts:
        one = one_sequence(np.random.default_rng(42), seq_len, layout)
        store = impg_amd.Sequences.from_arrays([str(i) for i in range(n_seq)], [np.roll(one, 7919 * i).tobytes() for i in range(n_seq)])
        by_form = {}
        for form in stores:
            g.set_sequences(None)
            t0 = time.perf_counter()
            g.set_sequences(store, packed=form == "packed")
            attach = time.perf_counter() - t0
            leg = {"n_layout": layout, "store": form, "attach_seconds": attach, "fasta_store_bytes": int(g.counter("fasta_store_bytes")),
                   "fasta_store_packed": int(g.counter("fasta_store_packed")), "fasta_store_exception_runs": int(g.counter("fasta_store_exception_runs"))}
            device(ranges)
            dev = [device(ranges) for _ in range(3)]
            leg["text_bytes"] = dev[0][2]
            leg["seconds"] = spread([x[0] for x in dev])
            leg["seconds3"] = {k: spread([x[1][i] for x in dev]) for i, k in enumerate(("engine", "rows_merge", "text"))}
            pieces = piece_timing(device, ranges)
            leg["pieces"] = {k: v for k, v in pieces.items() if k != "per_piece"}
            leg["pieces"]["n"] = len(pieces["per_piece"])
            n_sub = args.ranges if dev[0][2] <= args.host_bytes else max(1, int(args.ranges * args.host_bytes / dev[0][2]))
            text = g.query_batch_fasta(ranges[:n_sub], p, merge_distance=d, raw=True)
            leg["checked"] = {"ranges": n_sub, "text_bytes": len(text), "crc32": zlib.crc32(text)}
            by_form[form] = leg
            del text
            out["legs"].append(leg)
            save()
            print(json.dumps(leg), flush=True)
        if len(by_form) == 2:
            b, k = by_form["bytes"], by_form["packed"]
            cmp = {"n_layout": layout, "texts_equal": b["checked"] == k["checked"], "store_bytes_packed_over_bytes": k["fasta_store_bytes"] / b["fasta_store_bytes"],
                   "attach_packed_over_bytes": k["attach_seconds"] / b["attach_seconds"],
                   "seconds_packed_over_bytes": k["seconds"]["median"] / b["seconds"]["median"],
                   "kernel_over_copy": {"bytes": b["pieces"]["kernel_over_copy"], "packed": k["pieces"]["kernel_over_copy"]}}
            out.setdefault("compared", []).append(cmp)
            save()
            print(json.dumps(cmp), flush=True)
            if not cmp["texts_equal"]:
                raise SystemExit("the two stores print different text")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--ranges", type=int, default=10_000)
    ap.add_argument("--host-bytes", type=float, default=6e9, help="text the host twin (and the equality check) is asked for at most")
    ap.add_argument("--out", default="profiles/fasta_probe.json")
    ap.add_argument("--store", default="bytes", help="bytes | packed: the store's form in HBM (comma-separated: one leg each)")
    ap.add_argument("--n-layout", default="scattered", help="scattered | runs: where the 2 %% of N lie (comma-separated: one leg each)")
    args = ap.parse_args()
    stores, layouts = args.store.split(","), args.n_layout.split(",")
    if set(stores) - {"bytes", "packed"} or set(layouts) - {"scattered", "runs"}:
        ap.error("--store takes bytes, packed; --n-layout takes scattered, runs")
    n_seq, seq_len = 200, 5_000_000
    rec, ops, sl = impg_amd.synth_paf(42, args.records, n_seq=n_seq, seq_len=seq_len)
    g = impg_amd.GpuImpg.from_records(rec, ops, sl)
    del rec, ops
    # an index built from records has no names: its sequences print, and are matched, as their ids
    bed = impg_amd.synth_bed(7, args.ranges, n_seq=n_seq, seq_len=seq_len, range_len=5000)
    ranges = np.zeros(args.ranges, dtype=impg_amd.RANGE_DTYPE)
    ranges["target_id"], ranges["start"], ranges["end"] = bed["target_id"], bed["start"], bed["end"]
    kw = dict(transitive=True, max_depth=2)
    p = impg_amd.make_params(**kw)
    d = 0
    if len(stores) * len(layouts) > 1:
        return store_legs(args, g, n_seq, seq_len, ranges, p, d, stores, layouts)
    rng = np.random.default_rng(42)
    one = one_sequence(rng, seq_len, layouts[0])
    t0 = time.perf_counter()
    store = impg_amd.Sequences.from_arrays([str(i) for i in range(n_seq)], [np.roll(one, 7919 * i).tobytes() for i in range(n_seq)])
    t1 = time.perf_counter()
    g.set_sequences(store, packed=stores[0] == "packed")
    t2 = time.perf_counter()
    out = {"index": {"records": args.records, "sequences": n_seq, "sequence_length": seq_len}, "ranges": args.ranges, "range_length": 5000,
           "leg": "-x -m 2", "merge_distance": d, "store": {"load_seconds": t1 - t0, "attach_seconds": t2 - t1, "bytes_in_hbm": g.counter("fasta_store_bytes")}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    null = os.open(os.devnull, os.O_WRONLY)

    def device(r):
        t0 = time.perf_counter()
        n, sec = g.query_batch_fasta(r, p, merge_distance=d, fd=null, timing=True)
        return time.perf_counter() - t0, sec, n

    device(ranges)
    dev = [device(ranges) for _ in range(3)]
    total = dev[0][2]
    out["device"] = {"text_bytes": total, "counters": {k: int(g.counter(k)) for k in FASTA_COUNTERS}, "seconds": spread([x[0] for x in dev]),
                     "seconds3": {k: spread([x[1][i] for x in dev]) for i, k in enumerate(("engine", "rows_merge", "text"))}}
    out["device"]["text_bytes_per_second"] = total / out["device"]["seconds"]["median"]
    save()
    print(json.dumps(out["device"]), flush=True)

    # ---- the write kernel against the copy of the same piece --------------------------------------------------------------
    out["pieces"] = piece_timing(device, ranges)
    save()
    print(json.dumps({k: v for k, v in out["pieces"].items() if k != "per_piece"}), flush=True)

    # ---- the route against the host twin, on ranges whose text the host can hold twice -------------------------------------
    n_host = args.ranges if total <= args.host_bytes else max(1, int(args.ranges * args.host_bytes / total))
    sub = ranges[:n_host]
    device(sub)
    dsub = [device(sub) for _ in range(3)]
    L = _lib.lib()
    text, ln = C.c_void_p(None), C.c_size_t(0)
    sec = (C.c_double * 3)()
    _lib.check(L.impg_gpu_query_batch_fasta(g._h, sub.ctypes.data, sub.size, C.byref(p), None, d, None, 0, C.byref(text), C.byref(ln), sec))

    def host():
        t0 = time.perf_counter()
        res = g.query_batch(sub, p, copy=False)
        t1 = time.perf_counter()
        ht, hn = C.c_void_p(None), C.c_size_t(0)
        _lib.check(L.impg_gpu_results_fasta(res._h, g._h, C.byref(p), d, 0, C.byref(ht), C.byref(hn)))
        t2 = time.perf_counter()
        del res
        return t2 - t0, [t1 - t0, t2 - t1], ht, hn.value

    libc = C.CDLL(None)
    libc.memcmp.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    hst, equal = [], True
    for _ in range(2):
        h = host()
        equal = equal and h[3] == ln.value and libc.memcmp(h[2], text, ln.value) == 0
        _lib.free(h[2])
        hst.append(h)
    _lib.free(text)
    out["routes"] = {"ranges": n_host, "text_bytes": ln.value, "texts_equal": equal, "device_seconds": spread([x[0] for x in dsub]),
                     "host_seconds": spread([x[0] for x in hst]),
                     "host_split": {k: spread([x[1][i] for x in hst]) for i, k in enumerate(("query_batch", "fasta_text"))}}
    out["routes"]["device_over_host"] = out["routes"]["device_seconds"]["median"] / out["routes"]["host_seconds"]["median"]
    out["routes"]["device_faster_beyond_spread"] = out["routes"]["device_seconds"]["max"] < out["routes"]["host_seconds"]["min"]
    save()
    print(json.dumps(out["routes"]), flush=True)
    if not equal:
        raise SystemExit("the two routes print different text")


if __name__ == "__main__":
    main()
