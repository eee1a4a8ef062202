#!/usr/bin/env python3
"""Per-call latency of the trait-shaped calls on the headline index: impg_gpu_query (one range, no transitive),
query_transitive_bfs / _dfs and the MultiImpg worklists of either end, alone and in small batches.  Beside every transitive
row: the oracle's time for the same calls on one thread, and what the walk's counters did over the row.  Then a 1 000-range
MultiImpg `-m 3` batch under walk_kernel 1 and 0 (the bound, if any, in Engine::walk_applicable comes from these two).

--no-oracle leaves the oracle column out (its index of the headline file takes a while to build)."""
import os, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import impg_amd
with_oracle = "--no-oracle" not in sys.argv
paf = os.path.join(tempfile.gettempdir(), "impg_synth_1000000_seed42.paf")
if not os.path.exists(paf):
    impg_amd.synth_paf_text(paf, 42, 1_000_000)
g = impg_amd.GpuImpg.from_paf(paf)
bed = impg_amd.synth_bed(7, 4096)
ranges = np.zeros(len(bed), dtype=impg_amd.RANGE_DTYPE)
ranges["target_id"] = [g.seq_id(impg_amd.synth_seq_name(int(t))) for t in bed["target_id"]]
ranges["start"], ranges["end"] = bed["start"], bed["end"]
c = None
if with_oracle:
    from oracle import oracle as o
    c = o.OracleIndex(paf_paths=[paf], preparse=True)
    assert [c.seq_name(i) for i in range(4)] == [g.seq_name(i) for i in range(4)]


def oracle_us(kw, lo, n):
    """the oracle's time for ranges [lo, lo + n), one thread, microseconds"""
    if c is None or not kw.get("transitive"):
        return None
    r = ranges[lo:lo + n]
    return c.bench(r["target_id"], r["start"], r["end"], o.make_params(**kw), threads=1)[2] * 1e6


def counters():
    return g.counter("walk_launches"), g.counter("walk_fallbacks")


for label, kw in (("query", dict()), ("bfs -m 3", dict(transitive=True, max_depth=3)),
                  ("dfs -m 2", dict(transitive=True, dfs=True, max_depth=2)),
                  ("bfs3 multi", dict(transitive=True, max_depth=3, multi_impg=True)),
                  ("dfs3 multi", dict(transitive=True, dfs=True, max_depth=3, multi_impg=True)),
                  # the shape the per-query walk does not take (the batch engine answers it)
                  ("bfs3 cigar", dict(transitive=True, max_depth=3, store_cigar=True))):
    p = impg_amd.make_params(**kw)
    declined = label == "bfs3 cigar"
    for nb in ((1,) if declined else (1, 8, 64)):
        t0 = time.perf_counter()
        g.query_batch(ranges[:nb], p)
        slow = declined or time.perf_counter() - t0 > 0.2  # (answered by the batch engine, up to seconds a call: a few calls only)
        reps = 3 if slow else (200 if nb == 1 else 50)
        for _ in range(0 if slow else 4):
            g.query_batch(ranges[:nb], p)
        before = counters()
        times, rows = [], 0
        for k in range(reps):
            lo = (k * nb) % 4000
            t0 = time.perf_counter()
            r = g.query_batch(ranges[lo:lo + nb], p, copy=False)
            times.append(time.perf_counter() - t0)
            rows += r.total
        after = counters()
        n_or = min(reps, 3) if nb == 1 else 1
        orc = [oracle_us(kw, (k * nb) % 4000, nb) for k in range(n_or)]
        print("%-10s batch %2d: %10.1f us per call (min %.1f, median %.1f, max %.1f over %d), %7.0f rows per call | oracle, one thread: %s | walk launches +%d fallbacks +%d"
              % (label, nb, 1e6 * sum(times) / reps, 1e6 * min(times), 1e6 * float(np.median(times)), 1e6 * max(times), reps, rows / reps,
                 "-" if orc[0] is None else "%.1f us per call (first %d calls)" % (sum(orc) / n_or, n_or), after[0] - before[0], after[1] - before[1]), flush=True)

# a large MultiImpg batch under either engine
p = impg_amd.make_params(transitive=True, max_depth=3, multi_impg=True)
for walk_kernel in (1, 0):
    g.set_option("walk_kernel", walk_kernel)
    before = counters()
    t0 = time.perf_counter()
    st, cnt, ck = g.query_batch_stats(ranges[:1000], p)
    dt = time.perf_counter() - t0
    after = counters()
    print("bfs3 multi batch 1000, walk_kernel %d: %10.1f ms (engine %.1f ms), %d rows | walk launches +%d fallbacks +%d"
          % (walk_kernel, dt * 1e3, st.ms_total, int(cnt.sum()), after[0] - before[0], after[1] - before[1]), flush=True)
g.set_option("walk_kernel", 1)
