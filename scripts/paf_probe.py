"""Device PAF against the host route on the headline index: impg_gpu_query_batch_paf (query, merge, the merged CIGARs fused
and the text on the device) against query_batch(store_cigar=True) + .paf(fmt="paf") (rows and ops across PCIe, the fold
and snprintf on host threads), in one process.

  python scripts/paf_probe.py [--records 1000000] [--ranges 10000] [--out profiles/paf_probe.json]

Legs: plain and -x -m 2, each at d = 0 and d = 1000; one warm-up, then three runs of each route: the median and the
spread (min .. max), the device route with its seconds3 split {engine, rows + CIGARs + merge + elements + scan, text},
and the text bytes per second of either route.  Both texts are hashed and must be equal.  Then the cg passes' group
width: the device route's last two stages at option paf_group_log2 = 2 .. 6, on both legs at d = 0.  The json is rewritten
after every leg, so a run that is cut short leaves what it measured."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import impg_amd  # noqa: E402

LEGS = [("plain", dict()), ("-x -m 2", dict(transitive=True, max_depth=2))]
PAF_COUNTERS = ("paf_rows", "paf_runs", "paf_joins_contiguous", "paf_joins_gap", "paf_ops_read", "paf_ops_printed", "paf_through_rows",
                "paf_text_pieces")


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--ranges", type=int, default=10_000)
    ap.add_argument("--chunk-ranges", type=int, default=0, help="ranges per chunk of either route (0: the whole batch; set when a leg's op pool does not fit)")
    ap.add_argument("--out", default="profiles/paf_probe.json")
    args = ap.parse_args()
    n_seq, seq_len = 200, 5_000_000
    rec, ops, sl = impg_amd.synth_paf(42, args.records, n_seq=n_seq, seq_len=seq_len)
    g = impg_amd.GpuImpg.from_records(rec, ops, sl)
    del rec, ops
    bed = impg_amd.synth_bed(7, args.ranges, n_seq=n_seq, seq_len=seq_len, range_len=5000)
    ranges = np.zeros(args.ranges, dtype=impg_amd.RANGE_DTYPE)
    ranges["target_id"], ranges["start"], ranges["end"] = bed["target_id"], bed["start"], bed["end"]
    rnames = ["r%d" % i for i in range(args.ranges)]
    g.set_option("chunk_ranges", args.chunk_ranges)
    out = {"index": {"records": args.records, "sequences": n_seq, "sequence_length": seq_len}, "ranges": args.ranges, "range_length": 5000,
           "chunk_ranges": args.chunk_ranges, "runs": 3, "legs": [], "group_width": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    def device(p, d):
        t0 = time.perf_counter()
        text, sec = g.query_batch_paf(ranges, p, merge_distance=d, range_names=rnames, timing=True, raw=True)
        dt = time.perf_counter() - t0
        return dt, sec, hashlib.sha256(text).hexdigest(), len(text), text.count(b"\n")

    def host(kw, d):
        p = impg_amd.make_params(store_cigar=True, **kw)
        t0 = time.perf_counter()
        res = g.query_batch(ranges, p, copy=False)
        t1 = time.perf_counter()
        text = res.paf(rnames, merge_distance=d, params=p, fmt="paf", raw=True)
        t2 = time.perf_counter()
        del res
        return t2 - t0, [t1 - t0, t2 - t1], hashlib.sha256(text).hexdigest()

    for name, kw in LEGS:
        p = impg_amd.make_params(**kw)
        for d in (0, 1000):
            device(p, d)
            dev = [device(p, d) for _ in range(3)]
            tally = {k: int(g.counter(k)) for k in PAF_COUNTERS}
            host(kw, d)
            hst = [host(kw, d) for _ in range(3)]
            leg = {"leg": name, "merge_distance": d, "text_bytes": dev[0][3], "lines": dev[0][4], "sha256": dev[0][2],
                   "texts_equal": all(x[2] == dev[0][2] for x in dev + hst), "counters": tally,
                   "device_seconds": spread([x[0] for x in dev]),
                   "device_seconds3": {k: spread([x[1][i] for x in dev]) for i, k in enumerate(("engine", "rows_merge_elements_scan", "text"))},
                   "host_seconds": spread([x[0] for x in hst]),
                   "host_split": {k: spread([x[1][i] for x in hst]) for i, k in enumerate(("query_batch_store_cigar", "paf_text"))}}
            leg["device_over_host"] = leg["device_seconds"]["median"] / leg["host_seconds"]["median"]
            leg["device_faster_beyond_spread"] = leg["device_seconds"]["max"] < leg["host_seconds"]["min"]
            leg["device_text_bytes_per_second"] = leg["text_bytes"] / leg["device_seconds"]["median"]
            leg["host_text_bytes_per_second"] = leg["text_bytes"] / leg["host_seconds"]["median"]
            out["legs"].append(leg)
            save()
            print(json.dumps(leg), flush=True)
            if not leg["texts_equal"]:
                raise SystemExit("the two routes print different text")
    for name, kw in LEGS:
        p = impg_amd.make_params(**kw)
        for lg in (2, 3, 4, 5, 6):
            g.set_option("paf_group_log2", lg)
            device(p, 0)
            runs = [device(p, 0) for _ in range(3)]
            row = {"leg": name, "lanes_per_element": 1 << lg, "ops_per_row": g.counter("paf_ops_read") / max(1, g.counter("paf_rows")),
                   "rows_merge_elements_scan_seconds": spread([x[1][1] for x in runs]), "text_seconds": spread([x[1][2] for x in runs])}
            out["group_width"].append(row)
            save()
            print(json.dumps(row), flush=True)
    g.set_option("paf_group_log2", 2)


if __name__ == "__main__":
    main()
