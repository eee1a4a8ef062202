#!/usr/bin/env python3
"""The waves of lookup_count_coop_kernel by the path they took, for any bench.py workload: runs bench.py's main() in this
process with option lookup_stats 1 (one step, no extras), keeps hold of the index it builds and reads the three wave counters
when it is done.  The step's time is printed beside them, but under lookup_stats every wave adds to one word: it is no timing.
usage: python scripts/lookup_coop_shares.py <out.jsonl> [bench.py arguments, e.g. --workload skewed]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import impg_amd  # noqa: E402

KEYS = ("lookup_coop_waves", "lookup_lane_waves_mixed", "lookup_lane_waves_span")


def main():
    out_path, args = sys.argv[1], sys.argv[2:]
    seen = []
    set_option = impg_amd.GpuImpg.set_option

    def keep(self, key, value):  # (bench.py sets its engine options on the index it times)
        if self not in seen:
            seen.append(self)
        return set_option(self, key, value)

    impg_amd.GpuImpg.set_option = keep
    import bench
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "1", "--cpu-sample", "0", "--no-extras", "--no-tiers",
                "--engine-option", "lookup_stats=1"] + args
    sys.stdout.flush()
    with tempfile.TemporaryFile(mode="w+") as tmp:  # (bench.py writes its line to a copy of descriptor 1)
        keep1 = os.dup(1)
        os.dup2(tmp.fileno(), 1)
        try:
            bench.main()
        finally:
            os.dup2(keep1, 1)
            os.close(keep1)
        tmp.seek(0)
        line = tmp.read()
    res = json.loads(line.strip().splitlines()[-1])
    waves = {k: sum(g.counter(k) for g in seen) for k in KEYS}
    tot = max(sum(waves.values()), 1)
    rec = {"workload": " ".join(args) or "headline", "waves": waves, "share": {k: waves[k] / tot for k in KEYS},
           "ms_per_step_under_lookup_stats": res["ms_per_step"], "self_check": res["self_check"]}
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
