#!/bin/bash
# Occupancy grids on a batch (tools/batch_grid.py): (a) grid() of one agent row per scene, grid() of every row, observe(), scan(), one
# tick and the torch sequence a caller had before (pedestrian channels only, from state_tensor()), alternated in three rounds of 50
# (--part grid); (b) run(50), scan(), observe() and restart_device() of the batch without grids on this build against the parent
# commit's build, alternated process by process (PARENT_LIB names the parent's libsfm_hip.so; skipped without it); and a kernel trace
# of 50 x (run(1), observe(), scan(), grid() of the agents, grid() of every row): one sfm_batch_grid_kernel launch of each form
# beside one observe, one scan and one tick.  Each step under its own time limit, chained with &&.
# Output: OUT_DIR/r19_batch_grid.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/grid_trace; OUT_DIR defaults to
# build/batch_grid (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_grid.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_grid}
out=$dir/r19_batch_grid.txt
tr=$dir/grid_trace
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
k.sort(key=lambda r: int(r["Start_Timestamp"]))
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
def line(name, d):
    d = sorted(d)
    if d:
        print(f"# {name}: {len(d)} launches, median {d[len(d) // 2]} ns, min {d[0]} ns, max {d[-1]} ns")
ticks = [dur(r) for r in k if "sfm_batch_tick_kernel" in r["Kernel_Name"]]
line("sfm_batch_tick_kernel (warm-up launches left out)", ticks[6:])
line("sfm_batch_observe_kernel", [dur(r) for r in k if "sfm_batch_observe_kernel" in r["Kernel_Name"]])
line("sfm_batch_scan_kernel, every row", [dur(r) for r in k if "sfm_batch_scan_kernel" in r["Kernel_Name"]])
grids = [dur(r) for r in k if "sfm_batch_grid_kernel" in r["Kernel_Name"]]
line("sfm_batch_grid_kernel, one agent row per scene", grids[0::2])
line("sfm_batch_grid_kernel, every row", grids[1::2])
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (b) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (b) the paths that existed, without grids: the parent's build and this build, alternated process by process (us per call, per round of 50)"
  echo "build    call                             round    us/call"
  for r in 1 2 3; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_grid.py --part existing --label parent &&
    timeout -k 10 240 python3 tools/batch_grid.py --part existing --label this || return 1
  done
}
echo "# tools/batch_grid.sh: occupancy grids on a batch (sfm_batch_set_grid, sfm_batch_grid, SFM_BATCH_PTR_GRID)" > "$out"
timeout -k 10 300 python3 tools/batch_grid.py --part grid >> "$out" 2>> "$err" &&
ab >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$tr" -o bg -- \
    python3 tools/batch_grid.py --part trace --ticks 50 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace --stats of the trace part (name, calls, total ns, average ns, min ns, max ns):"
  stats "$tr"
} >> "$out" || exit 1
