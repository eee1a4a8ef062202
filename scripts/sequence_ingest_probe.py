"""impg_gpu_index_load_sequences against the host route it stands beside, on a store of the benchmark's size.

  python scripts/sequence_ingest_probe.py [--bases 1000000000] [--repeats 3] [--out profiles/sequence_ingest_probe.json]

A generated FASTA of --bases bases (20 sequences, lines of 80, 2 % N in four long runs per sequence), plain and as BGZF
(blocks of 65 280 input bytes).  Every leg runs in a process of its own, so that its peak host RSS is its own:

  host:bytes / host:packed        Sequences.from_fasta + set_sequences on the plain file (the route before this one)
  device:FORM:plain / :bgzf       load_sequences

Each leg warms up on a small file first (code objects, the pinned pool), then times --repeats runs with a host clock around
the call, which ends in a device synchronise.  The device legs then run once more under IMPG_SEQ_INGEST_TIMING: per piece
the H2D copy between two events, the piece's groups of kernels between events of their own (summed: no host round trip
is inside a group), and the reader's total (memcpy or inflate).  kernels_over_copy = the pieces' summed kernel time over
their summed H2D time.  The json is rewritten after every leg."""
import argparse
import json
import os
import resource
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_SEQ = 20
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def names_lens(bases):
    per = bases // N_SEQ // 80 * 80
    return ["seq%02d" % i for i in range(N_SEQ)], [per] * N_SEQ


def write_inputs(folder, bases):
    names, lens = names_lens(bases)
    rng = np.random.default_rng(1)
    plain, bgz = os.path.join(folder, "seqs.fa"), os.path.join(folder, "seqs.fa.gz")
    one = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=lens[0])].copy()
    run = lens[0] // 200
    for k in range(4):
        at = lens[0] * k // 4 + 1000
        one[at:at + run] = ord("N")
    with open(plain, "wb") as f:
        for i, nm in enumerate(names):
            body = np.empty((lens[i] // 80, 81), dtype=np.uint8)
            body[:, :80] = np.roll(one, 1013 * i).reshape(-1, 80)
            body[:, 80] = 10
            f.write(b">%s generated\n" % nm.encode())
            f.write(body.tobytes())

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
    small = os.path.join(folder, "small.fa")
    with open(small, "wb") as f:
        f.write(b">seq00\n" + b"ACGTN" * 16 + b"\n")
    paf = os.path.join(folder, "index.paf")
    with open(paf, "w") as f:
        for (q, lq), (t, lt) in zip(zip(names, lens), list(zip(names, lens))[1:]):
            f.write("%s\t%d\t0\t1\t+\t%s\t%d\t0\t1\t1\t1\t60\tcg:Z:1=\n" % (q, lq, t, lt))
    return {"plain": plain, "bgzf": bgz, "small": small, "paf": paf, "plain_bytes": os.path.getsize(plain), "bgzf_bytes": os.path.getsize(bgz)}


def leg(args):
    import impg_amd
    from impg_amd import Sequences
    route, form, kind = (args.leg.split(":") + ["plain"])[:3]
    packed = form == "packed"
    g = impg_amd.GpuImpg.from_paf(os.path.join(args.folder, "index.paf"))
    small_paf = os.path.join(args.folder, "small.paf")
    with open(small_paf, "w") as f:
        f.write("seq00\t80\t0\t1\t+\tseq01\t80\t0\t1\t1\t1\t60\tcg:Z:1=\n")
    w = impg_amd.GpuImpg.from_paf(small_paf)
    path = os.path.join(args.folder, "seqs.fa" if kind == "plain" else "seqs.fa.gz")
    small = os.path.join(args.folder, "small.fa")
    if route == "host":
        run = lambda h, p: h.set_sequences(Sequences.from_fasta(p), packed=packed)
    else:
        run = lambda h, p: h.load_sequences(p, packed=packed)
    run(w, small)  # warm-up
    out = {"leg": args.leg, "seconds": []}
    for _ in range(args.repeats):
        g.set_sequences(None)
        t0 = time.perf_counter()
        run(g, path)
        out["seconds"].append(time.perf_counter() - t0)
    out["median_seconds"] = statistics.median(out["seconds"])
    out["counters"] = {k: g.counter(k) for k in impg_amd.counter_keys() if k.startswith(("sequence_ingest_", "fasta_store_"))}
    if route == "device":
        with tempfile.TemporaryDirectory() as tmp:
            os.environ["IMPG_SEQ_INGEST_TIMING"] = os.path.join(tmp, "t.txt")
            t0 = time.perf_counter()
            run(g, path)
            total = time.perf_counter() - t0
            del os.environ["IMPG_SEQ_INGEST_TIMING"]
            lines = [ln.split() for ln in open(os.path.join(tmp, "t.txt"))]
        pieces = [(int(ln[0]), float(ln[1]), float(ln[2])) for ln in lines if ln[0] != "reader"]
        h2d, dev = sum(p[1] for p in pieces) * 1e-3, sum(p[2] for p in pieces) * 1e-3
        groups = {}
        for ln in lines:
            for name, ms in zip(("scan", "headers", "place", "runs"), ln[3:] if ln[0] != "reader" else []):
                groups[name] = groups.get(name, 0.0) + float(ms) * 1e-3
        out["split"] = {"seconds": total, "pieces": len(pieces), "reader_seconds": float([ln for ln in lines if ln[0] == "reader"][0][1]),
                        "h2d_seconds": h2d, "kernels_seconds": dev, "kernels_over_copy": dev / h2d if h2d else None,
                        "kernel_group_seconds": groups, "kernel_group_over_copy": {k: v / h2d for k, v in groups.items()} if h2d else None,
                        "h2d_bytes_per_second": sum(p[0] for p in pieces) / h2d if h2d else None}
    out["peak_rss_bytes"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    print("LEG " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1_000_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_ingest_probe.json"))
    ap.add_argument("--leg")
    ap.add_argument("--folder")
    ap.add_argument("--legs", default="device:bytes:plain,host:bytes,device:packed:plain,host:packed,device:bytes:bgzf,device:packed:bgzf")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    with tempfile.TemporaryDirectory() as folder:
        t0 = time.perf_counter()
        inputs = write_inputs(folder, args.bases)
        out = {"bases": sum(names_lens(args.bases)[1]), "sequences": N_SEQ, "line": 80, "plain_bytes": inputs["plain_bytes"],
               "bgzf_bytes": inputs["bgzf_bytes"], "repeats": args.repeats, "generate_seconds": time.perf_counter() - t0, "legs": []}
        for name in args.legs.split(","):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--folder", folder, "--repeats", str(args.repeats)],
                               capture_output=True, text=True)
            got = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            out["legs"].append(json.loads(got[0]) if got and r.returncode == 0 else {"leg": name, "failed": r.returncode, "stderr": r.stderr[-2000:]})
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
            print(name, out["legs"][-1].get("median_seconds"), flush=True)
            if r.returncode != 0:
                sys.exit("leg %s failed (%d): nothing more is started" % (name, r.returncode))


if __name__ == "__main__":
    main()
