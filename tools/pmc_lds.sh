#!/bin/bash
# LDS / VALU counters of one 16384^2 solve for two builds: the working tree and
# ab/$BASE/lib (tools/ab_build.sh).  Separate --pmc runs, no trace domain mixed in;
# then one rocprofv3 --kernel-trace --stats bench run each for the mean launch time.
# Output under $OUT/{tree,$BASE}/ (default bench_out_pmc_lds/ in the repository root);
# tools/pmc_lds_summary.py condenses it.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out_pmc_lds}
BASE=${BASE:-parent}
N=${N:-16384}
cd /tmp && export TMPDIR=/tmp
for b in $BASE tree; do
  O="$OUT/$b"; mkdir -p "$O"
  if [ $b = tree ]; then unset DYMU_LIBDIR; else export DYMU_LIBDIR=$R/ab/$b/lib; fi
  i=0
  for ctr in "SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAVES" "SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE" "SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU SQ_BUSY_CU_CYCLES"; do
    i=$((i+1))
    timeout -k 10 300 rocprofv3 --pmc $ctr --output-format csv -d "$O/p$i" -o run -- python3 "$R/tools/probe1.py" $N 1 > "$O/p$i.log" 2>&1 || { echo "!! pmc $b p$i rc=$?"; tail -20 "$O/p$i.log"; exit 1; }
  done
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt" -o run -- python3 "$R/bench.py" --steps 20 --warmup 5 > "$O/bench_rocprof.json" 2> "$O/bench_rocprof.err" || { echo "!! trace $b rc=$?"; tail -20 "$O/bench_rocprof.err"; exit 1; }
  find "$O/kt" -name "*kernel_stats.csv" -exec cp {} "$O/kernel_stats.csv" \;
  rm -rf "$O/kt"   # the per-dispatch trace is tens of MB: keep the stats only
  find "$O" -name "*agent_info.csv" -delete
  head -3 "$O/kernel_stats.csv"
done
