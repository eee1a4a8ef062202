"""impg_gpu_index_create_from_paf_streamed against the route it stands beside, on the headline's alignment file.

  python scripts/paf_ingest_probe.py [--records 1000000] [--repeats 3] [--out profiles/paf_ingest_probe.json]

The file is impg_synth_paf_text's (--records records of the benchmark's shape, about 600 bytes each), plain and as BGZF
(blocks of 65 280 input bytes, named .paf.gz so that the host route takes it for compressed).  Every leg runs in a process
of its own, so that its peak host RSS is its own:

  host:plain / host:bgzf          GpuImpg.from_paf(path)                      (the route before this one)
  device:plain / device:bgzf      GpuImpg.from_paf(path, ingest="device")

Each leg warms up on a small file first (code objects, the pinned pool), then times --repeats builds with a host clock
around the call (it ends with the index built and the first engine warm).  Then it builds once more with IMPG_BUILD_TIMING
-- and, on the device route, IMPG_PAF_INGEST_TIMING -- for the split: seconds to the hand-off (host route: line parser +
device tokenizer; device route: the streamed ingest, records home), the reader's and the name resolution's share, the H2D
copies and the three groups of kernels between events, the host's waits for the device, and the low-water mark of free
HBM sampled once a piece.  kernels_over_copy = the summed kernel time over the summed H2D time.  The json is rewritten after
every leg."""
import argparse
import json
import os
import re
import resource
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SHAPE = dict(n_seq=200, seq_len=5_000_000, target_span=10_000, n_blocks=100)


def write_inputs(folder, records):
    import impg_amd
    plain, bgz, small = (os.path.join(folder, n) for n in ("aln.paf", "aln.paf.gz", "small.paf"))
    impg_amd.synth_paf_text(plain, 42, records, **SHAPE)
    impg_amd.synth_paf_text(small, 43, 200, **SHAPE)

    def block(data):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = c.compress(data) + c.flush()
        return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(body) + 8 - 1) + body +
                struct.pack("<II", zlib.crc32(data), len(data)))
    with open(plain, "rb") as f, open(bgz, "wb") as out, ThreadPoolExecutor(16) as pool:
        while True:
            chunk = f.read(65280 * 1024)
            if not chunk:
                break
            for b in pool.map(block, [chunk[i:i + 65280] for i in range(0, len(chunk), 65280)]):
                out.write(b)
        out.write(BGZF_EOF)
    return {"plain_bytes": os.path.getsize(plain), "bgzf_bytes": os.path.getsize(bgz)}


def leg(args):
    import impg_amd
    route, kind = args.leg.split(":")
    path = os.path.join(args.folder, "aln.paf" if kind == "plain" else "aln.paf.gz")
    kw = dict(ingest="device") if route == "device" else {}
    w = impg_amd.GpuImpg.from_paf(os.path.join(args.folder, "small.paf"), **kw)  # warm-up
    del w
    out = {"leg": args.leg, "seconds": []}
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        g = impg_amd.GpuImpg.from_paf(path, **kw)
        out["seconds"].append(time.perf_counter() - t0)
        out["counters"] = {k: g.counter(k) for k in impg_amd.counter_keys() if k.startswith(("paf_ingest_", "build_", "tokenized_"))}
        out["records"] = g.num_records() if hasattr(g, "num_records") else None
        del g
    out["median_seconds"] = statistics.median(out["seconds"])
    out["spread_seconds"] = max(out["seconds"]) - min(out["seconds"])
    with tempfile.TemporaryDirectory() as tmp:  # the split: the library's own clocks, on stderr and in the timing file
        os.environ["IMPG_BUILD_TIMING"] = "1"
        if route == "device":
            os.environ["IMPG_PAF_INGEST_TIMING"] = os.path.join(tmp, "t.txt")
        err = os.path.join(tmp, "stderr.txt")
        keep = os.dup(2)
        with open(err, "wb") as f:
            os.dup2(f.fileno(), 2)
            try:
                t0 = time.perf_counter()
                g = impg_amd.GpuImpg.from_paf(path, **kw)
                total = time.perf_counter() - t0
                del g
            finally:
                os.dup2(keep, 2)
                os.close(keep)
        laps = [(m.group(1).strip(), float(m.group(2))) for m in re.finditer(r"\[build[^\]]*\] (.+?)\s+([0-9.]+) s", open(err).read())]
        split = {"seconds": total, "laps": laps}
        if route == "host":
            split["handoff_seconds"] = sum(s for name, s in laps if name.startswith(("parse PAF", "CIGAR text")))
        else:
            words = open(os.path.join(tmp, "t.txt")).read().split()
            v = {words[i]: float(words[i + 1]) for i in range(0, len(words) - 1, 2)}
            h2d, kern = v["h2d_ms"] * 1e-3, (v["scan_ms"] + v["names_ms"] + v["cigars_ms"]) * 1e-3
            split.update({"handoff_seconds": v["handoff_s"], "reader_seconds": v["reader_s"], "names_on_host_seconds": v["names_s"],
                          "pieces": int(v["pieces"]), "h2d_seconds": h2d,
                          "kernel_group_seconds": {"scan_heads_tag_lookup": v["scan_ms"] * 1e-3, "unknown_names_list": v["names_ms"] * 1e-3,
                                                   "patch_cigars_records": v["cigars_ms"] * 1e-3},
                          "kernels_seconds": kern, "kernels_over_copy": kern / h2d if h2d else None, "host_waits_seconds": v["wait_s"],
                          "free_hbm_start_bytes": int(v["free_start"]), "free_hbm_low_water_bytes": int(v["free_low"]),
                          "ingest_peak_hbm_bytes": int(v["free_start"] - v["free_low"]),
                          "ingest_peak_hbm_bytes_per_text_byte": (v["free_start"] - v["free_low"]) / os.path.getsize(os.path.join(args.folder, "aln.paf"))})
        out["split"] = split
    out["peak_rss_bytes"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    print("LEG " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paf_ingest_probe.json"))
    ap.add_argument("--leg")
    ap.add_argument("--folder")
    ap.add_argument("--legs", default="host:plain,device:plain,host:bgzf,device:bgzf")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    with tempfile.TemporaryDirectory() as folder:
        t0 = time.perf_counter()
        out = {"records": args.records, "shape": SHAPE, "repeats": args.repeats}
        out.update(write_inputs(folder, args.records))
        out["generate_seconds"] = time.perf_counter() - t0
        out["legs"] = []
        for name in args.legs.split(","):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--folder", folder, "--repeats", str(args.repeats)],
                               capture_output=True, text=True)
            got = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            out["legs"].append(json.loads(got[0]) if got and r.returncode == 0 else {"leg": name, "failed": r.returncode, "stderr": r.stderr[-2000:]})
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
            print(name, out["legs"][-1].get("median_seconds"), out["legs"][-1].get("seconds"), flush=True)
            if r.returncode != 0:
                sys.exit("leg %s failed (%d): nothing more is started" % (name, r.returncode))


if __name__ == "__main__":
    main()
