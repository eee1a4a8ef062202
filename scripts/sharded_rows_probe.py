"""The rows form of a sharded index against its counting form, on the headline workload (bench.py's: impg_synth_paf,
1e6 records, 200 sequences of 5 Mb, 100 000 ranges of 5 kb, -x -m 3) through one multi handle of w ranks that share
device 0 (as bench.py --world-sweep: constant work, the ranks' kernels on one GPU).

  python scripts/sharded_rows_probe.py [--worlds 1,2,4] [--steps 5] [--warmup 6] [--lanes 2] [--forms count,rows]
  python scripts/sharded_rows_probe.py --merge a.json b.json ...   (one line from the lines of single-world runs)

Per world, ms per step of
  rows    impg_gpu_query_batch_device (IMPG_ROWS_ATTRIBUTED; the handle freed inside the step)
  count   impg_gpu_query_batch_stats without per-range arrays (what bench.py times on a sharded index)
the final hop's bytes_hits_out (summed over the ranks) under each form, and the headline checksum recomputed from the
rows (impg_gpu_device_rows_check) against bench.HEADLINE_CHECKSUM.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import impg_amd  # noqa: E402
from impg_amd.index import HOP_PROFILE_FIELDS  # noqa: E402

N_SEQ, SEQ_LEN, RECORDS, RANGES = 200, 5_000_000, 1_000_000, 100_000
BYTES_HITS = HOP_PROFILE_FIELDS.index("bytes_hits_out")


def headline_checksum():
    with open(os.path.join(ROOT, "bench.py")) as f:
        for line in f:
            if line.startswith("HEADLINE_CHECKSUM"):
                return int(line.split("=")[1].split("#")[0].strip().replace("_", ""))
    return None


def workload():
    paf = os.path.join(tempfile.gettempdir(), "impg_synth_%d_seed42.paf" % RECORDS)  # (bench.py's file name: reused if there)
    if not os.path.exists(paf):
        impg_amd.synth_paf_text(paf + ".tmp", 42, RECORDS, n_seq=N_SEQ, seq_len=SEQ_LEN)
        os.replace(paf + ".tmp", paf)
    return paf


def leg(paf, ranges_ids, w, args, params, expect):
    t0 = time.perf_counter()
    mh = impg_amd.GpuImpg.from_paf(paf, devices=[0] * w, lanes=args.lanes)
    build_s = time.perf_counter() - t0
    ids = np.array([mh.seq_id(impg_amd.synth_seq_name(t)) for t in range(N_SEQ)], dtype=np.uint32)
    ranges = ranges_ids.copy()
    ranges["target_id"] = ids[ranges_ids["target_id"]]
    mh.set_option("pair_budget", 1 << 30)
    # (bench.py --world-sweep's chunks: a rank's block of the batch in one chunk per lane, at most 50 000 ranges)
    mh.set_option("chunk_ranges", max(1, min(50000, (len(ranges) + w * args.lanes - 1) // (w * args.lanes))))

    def count():
        return mh.query_batch_stats(ranges, params, counts=False, checksums=False)[0].projected

    def rows(keep=False):
        dr = mh.query_batch_device(ranges, params)
        p = dr.projected
        if keep:
            return dr
        dr.free()
        return p

    out = {"world": w, "lanes": args.lanes, "index_build_s": build_s}
    for name, f in (("count", count), ("rows", rows)):
        if name not in args.forms.split(","):
            continue
        for _ in range(args.warmup):
            f()
        mh.hop_profile(reset=True)
        t0 = time.perf_counter()
        proj = [f() for _ in range(args.steps)]
        dt = time.perf_counter() - t0
        prof = mh.hop_profile(reset=True) / max(1, args.steps)  # [w][8 hops][12]
        hops = int((prof[:, :, 0].sum(axis=0) > 0).sum())
        out[name] = {"ms_per_step": dt * 1e3 / args.steps, "projected_per_step": proj[-1], "hops": hops,
                     "bytes_hits_out_per_hop": [float(x) for x in prof[:, :hops, BYTES_HITS].sum(axis=0)],
                     "final_hop_bytes_hits_out": float(prof[:, hops - 1, BYTES_HITS].sum()) if hops else 0.0}
    dr = rows(keep=True)
    t0 = time.perf_counter()
    cnt, ck = dr.check()
    check_ms = (time.perf_counter() - t0) * 1e3
    parts = dr.parts()
    held = sum(int(d.n_slots) * 24 + int(d.n_frontier) * 16 for d in parts)  # (query id + source + four coordinates a slot)
    t0 = time.perf_counter()
    dr.free()
    free_ms = (time.perf_counter() - t0) * 1e3
    cks = int(ck.sum(dtype=np.uint64))
    out["rows_check"] = {"sum_of_per_range_checksums": cks, "expected": expect, "equal": cks == expect,
                         "rows": int(cnt.sum()), "parts": len(parts), "bytes_in_hbm": held, "check_ms": check_ms, "free_ms": free_ms}
    if "count" in out and "rows" in out:
        out["rows_over_count"] = out["rows"]["ms_per_step"] / out["count"]["ms_per_step"]
    del mh
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="1,2,4")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--forms", default="count,rows", help="the forms timed (a profiling run takes one)")
    ap.add_argument("--merge", nargs="*", default=None, help="files of single-world lines: print them as one line")
    args = ap.parse_args()
    if args.merge is not None:
        legs = []
        for fn in args.merge:
            with open(fn) as f:
                legs += json.loads(f.read().strip().splitlines()[-1])["legs"]
        print(json.dumps({"probe": "sharded_rows_probe", "legs": legs,
                          "headline_checksum_equal_at_every_world": all(x["rows_check"]["equal"] for x in legs)}))
        return
    paf = workload()
    bed = impg_amd.synth_bed(7, RANGES, n_seq=N_SEQ, seq_len=SEQ_LEN, range_len=5000)
    ranges = np.zeros(RANGES, dtype=impg_amd.RANGE_DTYPE)
    ranges["target_id"], ranges["start"], ranges["end"] = bed["target_id"], bed["start"], bed["end"]
    params = impg_amd.make_params(transitive=True, max_depth=3)
    expect = headline_checksum()
    legs = [leg(paf, ranges, int(w), args, params, expect) for w in args.worlds.split(",")]
    print(json.dumps({"probe": "sharded_rows_probe", "workload": "headline: %d records, %d ranges, -x -m 3; a multi handle of w ranks on "
                      "device 0" % (RECORDS, RANGES), "steps": args.steps, "warmup": args.warmup, "legs": legs,
                      "headline_checksum_equal_at_every_world": all(x["rows_check"]["equal"] for x in legs)}))


if __name__ == "__main__":
    main()
