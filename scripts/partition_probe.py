#!/usr/bin/env python3
"""Per-window cost of `impg partition`: (a) the device-state session, (b) the host-state session, (c) the loop a caller
writes against the query interface alone -- GpuImpg.query_transitive_bfs under a mask prepared anew every window, the
algebra in tests/partition_ref.py.  (c)'s query-call time (mask conversion, upload, query, row copy) is the baseline
and is reported apart from its Python algebra time.  Writes profiles/partition_probe.json.

Workload: impg_synth_paf_text, 2 x 10^5 records, default sequence table; -w 100000 -d 10000 -m 3, BFS, longest; the
first --windows windows (default 2000).  Every leg is timed per window with the device idle before and after (each call
synchronises); means over the first and the last tenth of the windows, where the mask has grown."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import impg_amd  # noqa: E402
from tests import partition_ref as pr  # noqa: E402

W, D, DEPTH = 100_000, 10_000, 3


def tenths(ms):
    k = max(1, len(ms) // 10)
    return dict(first_tenth_ms=sum(ms[:k]) / k, last_tenth_ms=sum(ms[-k:]) / k, windows=len(ms))


def session_leg(g, n_windows, host):
    s = g.partition_session(W, D, impg_amd.make_params(transitive=True, max_depth=DEPTH), state_on_host=host)
    ms, rows, mask = [], [], []
    try:
        while len(ms) < n_windows:
            ws = s.next_windows()
            if not ws:
                break
            for w in ws:
                t = time.perf_counter()
                out = s.window(*w)
                ms.append((time.perf_counter() - t) * 1e3)
                rows.append(len(out))
                if len(ms) >= n_windows:
                    break
            if len(ms) % 200 < len(ws) or len(ms) >= n_windows:
                mask.append((len(ms), sum(len(v) for v in s.regions().get("masked").values())))
        r = tenths(ms)
        r.update(out_rows_per_window=sum(rows) / max(1, len(rows)), mask_ranges=mask,
                 launches_per_window=s.counter("step_launches") / max(1, s.counter("windows")),
                 walk_windows=s.counter("walk_windows"), mask_uploads=s.counter("mask_uploads"), rows_to_host=s.counter("rows_to_host"))
        return r
    finally:
        s.close()


def caller_leg(g, n_windows):
    n = g.num_seqs()
    lens = [g.seq_len(q) for q in range(n)]
    ref = pr.Ref(lens)
    q_ms, a_ms, rows = [], [], []
    while len(q_ms) < n_windows:
        ws = ref.select("longest", W)
        if not ws:
            break
        for s, a, b in ws:
            t0 = time.perf_counter()
            mask = impg_amd.prepare_mask({q: (lens[q], ref.masked.get(q)) for q in range(n)})
            res = g.query_transitive_bfs(s, a, b, masked_regions=mask, max_depth=DEPTH)
            t1 = time.perf_counter()
            out = ref.apply([(int(r["query_id"]), int(r["q_first"]), int(r["q_last"])) for r in res], D, 3000, 3000)
            t2 = time.perf_counter()
            q_ms.append((t1 - t0) * 1e3)
            a_ms.append((t2 - t1) * 1e3)
            rows.append(len(res))
            if len(q_ms) >= n_windows:
                break
    r = dict(query_call=tenths(q_ms), python_algebra=tenths(a_ms), query_rows_per_window=sum(rows) / max(1, len(rows)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=2000)
    ap.add_argument("--records", type=int, default=200_000)
    ap.add_argument("--caller-windows", type=int, default=None, help="windows of leg (c) (default: --windows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition_probe.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "probe.paf")
        impg_amd.synth_paf_text(path, 42, a.records)
        g = impg_amd.GpuImpg.from_paf(path)
        session_leg(g, 20, False)  # warm-up: engines, slabs, scratch buffers
        res = dict(workload=dict(records=a.records, window=W, merge_distance=D, max_depth=DEPTH, selection="longest"),
                   device_state=session_leg(g, a.windows, False), host_state=session_leg(g, a.windows, True),
                   caller_loop=caller_leg(g, a.caller_windows or a.windows))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
