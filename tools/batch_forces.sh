#!/bin/bash
# Force records on a batch (tools/batch_forces.py --part time: run, run_recorded, run_recorded_forces with the total and with all
# six, step-wise tick_forces, alternated), a kernel + memory-copy trace of run_recorded_forces, and an A/B of plain run(50) against
# another library build: each step under its own time limit, chained with &&.
# Output: OUT_DIR/r10_batch_forces.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/forces_trace; OUT_DIR defaults to
# build/batch_forces (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   bash tools/batch_forces.sh [OUT_DIR] [OTHER_LIB]      (OTHER_LIB: e.g. variants/libsfm_old.so, built from the previous commit)
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_forces}
other=${2:-}
out=$dir/r10_batch_forces.txt
tr=$dir/forces_trace
err=$dir/stderr.log
mkdir -p "$dir" "$tr"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
for kind in ("kernel_stats", "memory_copy_stats"):
    files = sorted(glob.glob(sys.argv[1] + f"/**/*{kind}.csv", recursive=True))
    if kind == "memory_copy_stats":
        print("# memory copies over the whole process (uploads, set-up, final downloads):" if files else "# no memory copies traced")
    for f in files:
        for r in csv.DictReader(open(f)):
            print(f"{r['Name'][:60]:<60} {r['Calls']:>6} {r['TotalDurationNs']:>12} {float(r['AverageNs']):>10.0f} {r['MinNs']:>8} {r['MaxNs']:>8}")
kt = sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True))
mt = sorted(glob.glob(sys.argv[1] + "/**/*memory_copy_trace.csv", recursive=True))
k = [r for f in kt for r in csv.DictReader(open(f))]
m = [r for f in mt for r in csv.DictReader(open(f))]
ticks = [r for r in k if "sfm_batch_tick_kernel<false, true, false>" in r["Kernel_Name"]]
if ticks:
    t0, t1 = min(int(r["Start_Timestamp"]) for r in ticks), max(int(r["End_Timestamp"]) for r in ticks)
    inside = lambda r: t0 <= int(r["Start_Timestamp"]) <= t1
    print(f"# between the first and the last of the {len(ticks)} recording launches: {sum(map(inside, m))} memory copies, "
          f"{sum(1 for r in k if inside(r) and r not in ticks)} other kernel launches")
PY
}
echo "# tools/batch_forces.sh: force records on a batch (sfm_batch_tick_forces, sfm_batch_run_recorded_forces)" > "$out"
timeout -k 10 300 python3 tools/batch_forces.py --part time >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d "$tr" -o bf -- \
    python3 tools/batch_forces.py --part trace --ticks 100 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace --memory-copy-trace --stats of the trace part (name, calls, total ns, average ns, min ns, max ns):"
  stats "$tr"
} >> "$out" || exit 1
if [ -n "$other" ]; then
  echo "# A/B of plain run(50) (tools/batch_forces.py --part plain), builds alternated: this build, then $other" >> "$out"
  for r in 0 1 2; do
    echo "== this build" >> "$out"
    timeout -k 10 120 python3 tools/batch_forces.py --part plain --rounds 2 >> "$out" 2>> "$err" || exit 1
    echo "== other build" >> "$out"
    SFM_LIB_PATH=$root/$other timeout -k 10 120 python3 tools/batch_forces.py --part plain --rounds 2 >> "$out" 2>> "$err" || exit 1
  done
fi
