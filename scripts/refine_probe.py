#!/usr/bin/env python3
"""Cost of `impg refine` on the headline index (impg_synth_paf_text seed 42, 10^6 records, default sequence table): 1 000 and
10 000 loci of 5 kb (impg_synth_bed seed 7) on the reference's defaults (--span-bp 1000, --max-extension 0.5,
--extension-step 1000, -d 0), plain and -x -m 2, level `sequence`.  Per run: wall time on the device route and with
support_on_host; per batch of the run (the passes, then the read of the winners' survivors) the candidates, the wall time of
the query call, the engine's HIP-event time inside it (stage clocks + row placement) and the wall time of the support; what
is left of the run's wall time is host work (the candidates of the next pass, the reduction, the records).  Every leg runs
once to warm up and is then timed --repeats times; the median run is reported.  Writes profiles/refine_probe.json."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import impg_amd  # noqa: E402


def leg(g, loci, kw, on_host, repeats):
    p = impg_amd.make_params(**kw)
    g.refine(loci, p, on_host=on_host)  # warm-up: engines, scratch, pooled rows
    runs = []
    for _ in range(repeats):
        before = g.counter("refine_rows_to_host")
        t = time.perf_counter()
        r = g.refine(loci, p, on_host=on_host)
        wall = time.perf_counter() - t
        q = sum(b["query_s"] for b in r.batch_times)
        s = sum(b["support_s"] for b in r.batch_times)
        runs.append(dict(wall_s=wall, query_s=q, engine_ms=sum(b["engine_ms"] for b in r.batch_times), support_s=s, host_s=wall - q - s,
                         passes=r.passes, candidates=r.candidates, parts=r.parts, rows_to_host=g.counter("refine_rows_to_host") - before,
                         batches=r.batch_times, extended=sum(1 for x in r.records if x["left_extension"] or x["right_extension"]),
                         mean_support=sum(x["support_count"] for x in r.records) / max(1, len(r.records))))
    runs.sort(key=lambda x: x["wall_s"])
    med = runs[len(runs) // 2]
    med["wall_s_all"] = [x["wall_s"] for x in runs]
    med["wall_s_median"] = statistics.median(med["wall_s_all"])
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--loci", type=int, nargs="+", default=[1000, 10_000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_probe.json"))
    a = ap.parse_args()
    res = dict(workload=dict(records=a.records, locus_bp=5000, span_bp=1000, max_extension=0.5, extension_step=1000, merge_distance=0,
                             level="sequence", repeats=a.repeats), runs=[])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "probe.paf")
        impg_amd.synth_paf_text(path, 42, a.records)
        g = impg_amd.GpuImpg.from_paf(path)
        for n in a.loci:
            bed = impg_amd.synth_bed(7, n, range_len=5000)
            loci = [(g.seq_id(impg_amd.synth_seq_name(int(r["target_id"]))), int(r["start"]), int(r["end"])) for r in bed]
            for name, kw in (("plain", dict()), ("-x -m 2", dict(transitive=True, max_depth=2))):
                for on_host in (False, True):
                    r = leg(g, loci, kw, on_host, a.repeats)
                    r.update(loci=n, query=name, route="support_on_host" if on_host else "device")
                    res["runs"].append(r)
                    print("%6d loci %-8s %-15s wall %.3f s (query %.3f, engine %.1f ms, support %.3f, host %.3f) passes %d candidates %d rows_to_host %d"
                          % (n, name, r["route"], r["wall_s"], r["query_s"], r["engine_ms"], r["support_s"], r["host_s"], r["passes"], r["candidates"],
                             r["rows_to_host"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
