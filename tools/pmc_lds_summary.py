"""Condense a tools/pmc_lds.sh run into one JSON: per build the pass kernel's
counter totals over one 16384^2 solve, its dispatch count and its mean launch time
from the kernel-trace stats.  (No top-level "kernel" key: bench.py's roofline reads
the HBM-traffic summaries profiles/pmc_*.json of tools/pmc_summary.py, which this
is not.)
usage: python tools/pmc_lds_summary.py bench_out_pmc_lds OUT.json BUILD [BUILD ...]"""
import collections
import csv
import glob
import json
import sys

KERN = "k_fim_pass_dyn<16, true, false>"


def build(root):
    tot, disp, name = collections.Counter(), collections.defaultdict(set), None
    for f in sorted(glob.glob(root + "/p*/**/*counter_collection.csv", recursive=True)):
        for r in csv.DictReader(open(f)):
            if KERN in r["Kernel_Name"]:
                name = r["Kernel_Name"]
                tot[r["Counter_Name"]] += float(r["Counter_Value"])
                disp[r["Counter_Name"]].add(r["Dispatch_Id"])
    out = {"kernel_name": name, "dispatches": max((len(v) for v in disp.values()), default=0),
           "counters": dict(tot)}
    for r in csv.DictReader(open(root + "/kernel_stats.csv")):
        if KERN in r["Name"]:
            out["trace"] = {"calls": int(r["Calls"]), "avg_launch_us": float(r["AverageNs"]) / 1e3,
                            "total_ms": float(r["TotalDurationNs"]) / 1e6}
    return out


def main():
    root, dst, builds = sys.argv[1], sys.argv[2], sys.argv[3:]
    out = {"workload": "one 16384^2 config-3 solve (tools/probe1.py) per --pmc run; trace: "
                       "bench.py --steps 20 --warmup 5 under rocprofv3 --kernel-trace --stats",
           "builds": {b: build(root + "/" + b) for b in builds}}
    json.dump(out, open(dst, "w"), indent=1)
    for b, d in out["builds"].items():
        print(b, d["dispatches"], d.get("trace"), {k: "%.4g" % v for k, v in d["counters"].items()})


if __name__ == "__main__":
    main()
