#!/usr/bin/env python3
"""Where a wave of the count kernels spends its life (library built with -DIMPG_LOOKUP_CLOCKS: scripts/build_phase_lib.sh with
EXTRA=-DIMPG_LOOKUP_CLOCKS, IMPG_GPU_LIB pointing at it): s_memtime at the dependency boundaries of lookup_count_lane_kernel
(option lookup_coop 0) and of lookup_count_coop_kernel (1), each wait drained first, summed over the waves of every 16th
block of one headline step, all levels.
usage: IMPG_GPU_LIB=impg_amd/libimpg_lkclk.so python scripts/lookup_clocks.py [ranges] > profiles/lookup_coop_clocks.json"""
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import impg_amd  # noqa: E402

LANE = ["perm + record + segment descriptor", "sample search (4-ary, global)", "block search (4-ary, global)", "window walk (global)", "stores"]
COOP = ["perm + record + segment descriptor", "reductions + wave searches (global)", "staging into LDS", "lane searches (LDS)",
        "window walk (LDS)", "stores"]


def main():
    n_ranges = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    fn = impg_amd.lib().impg_gpu_debug_lookup_clocks
    fn.argtypes = [C.c_void_p]
    n_seq, seq_len, records = 200, 5_000_000, 1_000_000
    paf = os.path.join(tempfile.gettempdir(), "impg_synth_%d_seed42.paf" % records)
    if not os.path.exists(paf):
        impg_amd.synth_paf_text(paf, 42, records, n_seq=n_seq, seq_len=seq_len)
    g = impg_amd.GpuImpg.from_paf(paf)
    g.set_option("chunk_ranges", max(50000, n_ranges))
    g.set_option("pair_budget", 3 << 30)
    bed = impg_amd.synth_bed(7, n_ranges, n_seq=n_seq, seq_len=seq_len, range_len=5000)
    ranges = np.zeros(n_ranges, dtype=impg_amd.RANGE_DTYPE)
    ids = np.array([g.seq_id(impg_amd.synth_seq_name(t)) for t in range(n_seq)], dtype=np.uint32)
    ranges["target_id"], ranges["start"], ranges["end"] = ids[bed["target_id"]], bed["start"], bed["end"]
    params = impg_amd.make_params(transitive=True, max_depth=3)
    buf = (C.c_uint64 * 16)()
    out = {"ranges": n_ranges, "sampled": "full waves of every 16th block, every level of one step"}
    for coop in (0, 1):
        g.set_option("lookup_coop", coop)
        # (the waves by path come from a step of their own: under lookup_stats every wave adds to one word, which the clocks would see)
        g.set_option("lookup_stats", 1)
        before = {k: g.counter(k) for k in ("lookup_coop_waves", "lookup_lane_waves_mixed", "lookup_lane_waves_span")}
        g.query_batch_stats(ranges, params, counts=False, checksums=False)          # warm-up
        by_path = {k: g.counter(k) - before[k] for k in before}
        g.set_option("lookup_stats", 0)
        fn(C.cast(buf, C.c_void_p))                                                 # clear
        st, _, _ = g.query_batch_stats(ranges, params, counts=False, checksums=False)
        fn(C.cast(buf, C.c_void_p))
        names, base = (COOP, 6) if coop else (LANE, 0)
        n = buf[base + len(names)]
        tot = sum(buf[base + i] for i in range(len(names)))
        o = {"waves_sampled": int(n), "cycles_per_wave": tot / max(n, 1), "ms_lookup": st.ms_lookup, "projected": int(st.projected),
             "phases": [{"phase": names[i], "cycles_per_wave": buf[base + i] / max(n, 1), "share": buf[base + i] / max(tot, 1)} for i in range(len(names))]}
        if coop:
            o["lane_body_waves_sampled"] = int(buf[14])
            o["lane_body_cycles_per_wave_behind_the_loads"] = buf[13] / max(buf[14], 1)
            o["waves_by_path"] = by_path
        out["lookup_count_coop_kernel" if coop else "lookup_count_lane_kernel"] = o
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
