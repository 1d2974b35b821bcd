#!/bin/bash
# Bird's-eye grids around the vehicles of a batch (tools/batch_vehicle_grid.py): (a) run(50), grid() and scan_vehicles() on this
# build against the parent commit's build, alternated process by process in three rounds, both orders of the pair (PARENT_LIB names
# the parent's libsfm_hip.so; skipped without it); (b) grid_vehicles() with one ego vehicle per scene at 32 x 32 and at 48 x 20 with a
# forward centre and with every vehicle at 32 x 32, beside grid() of one agent row per scene and scan_vehicles() at 64 rays (--part
# grid); (c) the torch sequence a caller had before beside the one launch (--part torch); and a kernel trace of 50 grid_vehicles()
# calls of each form, in a run of its own (no counters in that run).  Each step under its own time limit, chained with &&.
# Output: OUT_DIR/r25_batch_vehicle_grid.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/vehicle_grid_trace; OUT_DIR
# defaults to build/batch_vehicle_grid (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_vehicle_grid.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_vehicle_grid}
out=$dir/r25_batch_vehicle_grid.txt
tr=$dir/vehicle_grid_trace
err=$dir/stderr.log
mkdir -p "$dir" "$tr"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
k = [r for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)) for r in csv.DictReader(open(f))]
k = sorted((r for r in k if "sfm_batch_vehicle_grid_kernel" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
d = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in k][9:]          # (the 3 x 3 warm-up launches come first)
n = len(d) // 3
for j, name in enumerate(("e32: one ego per scene, 32 x 32", "e48: one ego per scene, 48 x 20", "a32: every vehicle, 32 x 32")):
    part = sorted(d[j * n:(j + 1) * n])
    if part:
        print(f"# sfm_batch_vehicle_grid_kernel, {name}: {len(part)} launches, median {part[len(part) // 2]} ns, min {part[0]} ns, max {part[-1]} ns")
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (a) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (a) run(50), 50 x grid() and 50 x scan_vehicles(): the parent's build and this build, alternated process by process (us per tick, us per call)"
  echo "build         B   N_b round    us/tick    us/grid    us/scan"
  for r in 1 2 3; do                                       # both orders of the pair: the process that runs first tends to be the faster one
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_vehicle_grid.py --part run --label parent &&
    timeout -k 10 240 python3 tools/batch_vehicle_grid.py --part run --label this &&
    timeout -k 10 240 python3 tools/batch_vehicle_grid.py --part run --label this &&
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_vehicle_grid.py --part run --label parent || return 1
  done
}
echo "# tools/batch_vehicle_grid.sh: bird's-eye grids around the vehicles of a batch (sfm_batch_set_vehicle_grid, sfm_batch_grid_vehicles)" > "$out"
ab >> "$out" 2>> "$err" &&
timeout -k 10 300 python3 tools/batch_vehicle_grid.py --part grid >> "$out" 2>> "$err" &&
timeout -k 10 300 python3 tools/batch_vehicle_grid.py --part torch >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$tr" -o vg -- \
    python3 tools/batch_vehicle_grid.py --part trace --ticks 50 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace of the trace part:"
  stats "$tr"
} >> "$out" || exit 1
