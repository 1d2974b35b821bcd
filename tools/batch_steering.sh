#!/bin/bash
# Steered pedestrians on a batch (tools/batch_steering.py): (a) the cost of the feature, run(50) with a quarter of the rows at
# kind 1 and a quarter at kind 2 against the same batch without steering (--part cost); (b) run(50) of the unsteered batch on this
# build against the parent commit's build, alternated process by process (PARENT_LIB names the parent's libsfm_hip.so; skipped
# without it); (c) the RL step: set_commands + run(1) and a command_tensor() write + run(1) against download, edit, upload, run(1)
# (--part step); and a kernel + memory-copy trace of steered ticks: each step under its own time limit, chained with &&.
# Output: OUT_DIR/r14_batch_steering.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/steering_trace; OUT_DIR
# defaults to build/batch_steering (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_steering.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_steering}
out=$dir/r14_batch_steering.txt
tr=$dir/steering_trace
err=$dir/stderr.log
mkdir -p "$dir" "$tr"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
for kind in ("kernel_stats", "memory_copy_stats"):
    files = sorted(glob.glob(sys.argv[1] + f"/**/*{kind}.csv", recursive=True))
    if kind == "memory_copy_stats":
        print("# memory copies over the whole process (uploads and set-up included):" if files else "# no memory copies traced")
    for f in files:
        for r in csv.DictReader(open(f)):
            print(f"{r['Name'][:60]:<60} {r['Calls']:>6} {r['TotalDurationNs']:>12} {float(r['AverageNs']):>10.0f} {r['MinNs']:>8} {r['MaxNs']:>8}")
kt = sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True))
mt = sorted(glob.glob(sys.argv[1] + "/**/*memory_copy_trace.csv", recursive=True))
k = [r for f in kt for r in csv.DictReader(open(f))]
m = [r for f in mt for r in csv.DictReader(open(f))]
ticks = [r for r in k if "sfm_batch_tick_kernel" in r["Kernel_Name"]]
if ticks:
    t0, t1 = min(int(r["Start_Timestamp"]) for r in ticks), max(int(r["End_Timestamp"]) for r in ticks)
    inside = lambda r: t0 <= int(r["Start_Timestamp"]) <= t1
    copies = [r for r in m if inside(r)]
    kinds = sorted({r.get("Direction", "?") for r in copies})
    names = sorted({r["Kernel_Name"][:70] for r in ticks})
    print(f"# {len(ticks)} tick launches ({'; '.join(names)}); between the first tick launch and the last: "
          f"{sum(1 for r in k if inside(r) and r not in ticks)} other kernel launches, {len(copies)} memory copies "
          f"({', '.join(kinds) or 'none'}: one per set_commands)")
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (b) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (b) run(50) without steering: the parent's build and this build, alternated process by process (us/tick per round of run(50))"
  echo "build         B   N_b round    us/tick  scene-ticks/s"
  for r in 1 2 3; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_steering.py --part run --label parent &&
    timeout -k 10 240 python3 tools/batch_steering.py --part run --label this || return 1
  done
}
echo "# tools/batch_steering.sh: steered pedestrians on a batch (sfm_batch_set_steering, sfm_batch_set_commands, sfm_batch_device_ptr)" > "$out"
timeout -k 10 300 python3 tools/batch_steering.py --part cost >> "$out" 2>> "$err" &&
ab >> "$out" 2>> "$err" &&
timeout -k 10 600 python3 tools/batch_steering.py --part step >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d "$tr" -o bs -- \
    python3 tools/batch_steering.py --part trace --ticks 50 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace --memory-copy-trace --stats of the trace part (name, calls, total ns, average ns, min ns, max ns):"
  stats "$tr"
} >> "$out" || exit 1
