#!/usr/bin/env python3
"""The visited update's groups by tier over one step of any bench.py workload: runs bench.py's main() in this process with
option update_stats 1 (one step, no warm-up, no extras), keeps hold of the index it builds and reads the update_* counters
and place_offsets_block_levels when it is done.  Under update_stats every update copies its words home: it is no timing.
usage: python scripts/update_tier_counts.py <out.jsonl> [bench.py arguments, e.g. --workload skewed]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import impg_amd  # noqa: E402

KEYS = ("update_lane_groups", "update_mid_groups", "update_wave_tiny_groups", "update_wave_small_groups", "update_wave_large_groups",
        "place_offsets_block_levels")


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
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0", "--cpu-sample", "0", "--no-extras", "--no-tiers",
                "--engine-option", "update_stats=1"] + args
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
    have = set(impg_amd.counter_keys())
    rec = {"workload": " ".join(args) or "headline", "groups": {k: sum(g.counter(k) for g in seen) for k in KEYS if k in have},
           "self_check": res["self_check"]}
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
