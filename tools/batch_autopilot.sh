#!/bin/bash
# The vehicle autopilot on a batch (tools/batch_autopilot.py): (a) run(50) of the batch with the autopilot never set on this build
# against the parent commit's build, alternated process by process in three rounds and in both orders (PARENT_LIB names the
# parent's libsfm_hip.so; skipped without it); (b) run(50) with 0, 1 and 4 vehicles per scene autopiloted, alternated in three
# rounds (--part pilot); (c) the path a caller had before -- observe_vehicles(), a torch IDM on the nearest pedestrian only, the
# commands written through vehicle_command_tensor(), run(1) -- beside the autopilot (--part old); and a kernel trace of run(50) with
# every vehicle autopiloted, in a run of its own: one sfm_batch_vehicle_autopilot_kernel launch per tick.  Each step under its own
# time limit, chained with &&.
# Output: OUT_DIR/r24_batch_autopilot.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/autopilot_trace; OUT_DIR
# defaults to build/batch_autopilot (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_autopilot.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_autopilot}
out=$dir/r24_batch_autopilot.txt
tr=$dir/autopilot_trace
err=$dir/stderr.log
mkdir -p "$dir" "$tr"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
k = [r for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)) for r in csv.DictReader(open(f))]
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
for name in ("sfm_batch_tick_kernel", "sfm_batch_vehicle_autopilot_kernel"):
    d = sorted(dur(r) for r in k if name in r["Kernel_Name"])
    if d:
        d = d[3:] if len(d) > 3 else d
        print(f"# {name}: {len(d)} launches, median {d[len(d) // 2]} ns, min {d[0]} ns, max {d[-1]} ns")
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (a) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (a) run(50), the autopilot never set: the parent's build and this build, alternated process by process (us/tick per round of run(50))"
  echo "build         B   N_b round    us/tick  scene-ticks/s"
  for r in 1 2 3; do                                       # both orders of the pair: the process that runs first tends to be the faster one
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_autopilot.py --part run --label parent &&
    timeout -k 10 240 python3 tools/batch_autopilot.py --part run --label this &&
    timeout -k 10 240 python3 tools/batch_autopilot.py --part run --label this &&
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_autopilot.py --part run --label parent || return 1
  done
}
echo "# tools/batch_autopilot.sh: the vehicle autopilot on a batch (sfm_batch_set_vehicle_autopilot)" > "$out"
ab >> "$out" 2>> "$err" &&
timeout -k 10 300 python3 tools/batch_autopilot.py --part pilot >> "$out" 2>> "$err" &&
timeout -k 10 300 python3 tools/batch_autopilot.py --part old >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$tr" -o ap -- \
    python3 tools/batch_autopilot.py --part trace --ticks 50 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace of the trace part:"
  stats "$tr"
} >> "$out" || exit 1
