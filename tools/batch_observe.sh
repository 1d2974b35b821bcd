#!/bin/bash
# Per-pedestrian observations on a batch (tools/batch_observe.py): (a) observe() with everything, observe() on the same crowds
# without geometry, and the torch sequence a caller had before (cdist, topk, gather from state_tensor()), alternated in three
# rounds of 50 observations (--part obs); (b) run(50) of the batch without observations on this build against the parent commit's
# build, alternated process by process (PARENT_LIB names the parent's libsfm_hip.so; skipped without it); and a kernel trace of
# 50 x (run(1), observe()): one sfm_batch_observe_kernel launch beside one sfm_batch_tick_kernel launch of the same batch.  Each
# step under its own time limit, chained with &&.
# Output: OUT_DIR/r15_batch_observe.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/observe_trace; OUT_DIR defaults
# to build/batch_observe (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_observe.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_observe}
out=$dir/r15_batch_observe.txt
tr=$dir/observe_trace
err=$dir/stderr.log
mkdir -p "$dir" "$tr"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_stats.csv", recursive=True)):
    for r in csv.DictReader(open(f)):
        print(f"{r['Name'][:72]:<72} {r['Calls']:>6} {r['TotalDurationNs']:>12} {float(r['AverageNs']):>10.0f} {r['MinNs']:>8} {r['MaxNs']:>8}")
k = [r for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)) for r in csv.DictReader(open(f))]
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
for name in ("sfm_batch_tick_kernel", "sfm_batch_observe_kernel"):
    d = sorted(dur(r) for r in k if name in r["Kernel_Name"])
    if d:
        d = d[3:] if name == "sfm_batch_tick_kernel" and len(d) > 3 else d
        print(f"# {name}: {len(d)} launches, median {d[len(d) // 2]} ns, min {d[0]} ns, max {d[-1]} ns")
ticks = [r for r in k if "sfm_batch_tick_kernel" in r["Kernel_Name"]]
if ticks:
    t0, t1 = min(int(r["Start_Timestamp"]) for r in ticks), max(int(r["End_Timestamp"]) for r in ticks)
    other = [r for r in k if t0 <= int(r["Start_Timestamp"]) <= t1 and "sfm_batch_tick_kernel" not in r["Kernel_Name"]
             and "sfm_batch_observe_kernel" not in r["Kernel_Name"]]
    print(f"# between the first tick launch and the last: {len(other)} launches that are neither a tick nor an observe")
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (b) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (b) run(50) without observations: the parent's build and this build, alternated process by process (us/tick per round of run(50))"
  echo "build         B   N_b round    us/tick  scene-ticks/s"
  for r in 1 2 3; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_observe.py --part run --label parent &&
    timeout -k 10 240 python3 tools/batch_observe.py --part run --label this || return 1
  done
}
echo "# tools/batch_observe.sh: per-pedestrian observations on a batch (sfm_batch_set_observation, sfm_batch_observe, sfm_batch_observation_ptr)" > "$out"
timeout -k 10 300 python3 tools/batch_observe.py --part obs >> "$out" 2>> "$err" &&
ab >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$tr" -o bo -- \
    python3 tools/batch_observe.py --part trace --ticks 50 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace --stats of the trace part (name, calls, total ns, average ns, min ns, max ns):"
  stats "$tr"
} >> "$out" || exit 1
