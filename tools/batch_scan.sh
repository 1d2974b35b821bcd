#!/bin/bash
# Range scans on a batch (tools/batch_scan.py): (a) scan() of one agent row per scene, scan() of every row, observe() and the torch
# sequence a caller had before (pedestrian discs only, from state_tensor()), alternated in three rounds of 50 (--part scan); (b)
# run(50) of the batch without scans on this build against the parent commit's build, alternated process by process (PARENT_LIB
# names the parent's libsfm_hip.so; skipped without it); and a kernel trace of 50 x (run(1), observe(), scan() of the agents, scan()
# of every row): one sfm_batch_scan_kernel launch of each form beside one observe and one tick.  Each step under its own time
# limit, chained with &&.
# Output: OUT_DIR/r17_batch_scan.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/scan_trace; OUT_DIR defaults to
# build/batch_scan (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_scan.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_scan}
out=$dir/r17_batch_scan.txt
tr=$dir/scan_trace
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
scans = [dur(r) for r in k if "sfm_batch_scan_kernel" in r["Kernel_Name"]]
line("sfm_batch_scan_kernel, one agent row per scene", scans[0::2])
line("sfm_batch_scan_kernel, every row", scans[1::2])
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (b) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (b) run(50) without scans: the parent's build and this build, alternated process by process (us/tick per round of run(50))"
  echo "build         B   N_b round    us/tick  scene-ticks/s"
  for r in 1 2 3; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_scan.py --part run --label parent &&
    timeout -k 10 240 python3 tools/batch_scan.py --part run --label this || return 1
  done
}
echo "# tools/batch_scan.sh: range scans on a batch (sfm_batch_set_scan, sfm_batch_scan, SFM_BATCH_PTR_SCAN)" > "$out"
timeout -k 10 300 python3 tools/batch_scan.py --part scan >> "$out" 2>> "$err" &&
ab >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$tr" -o bs -- \
    python3 tools/batch_scan.py --part trace --ticks 50 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace --stats of the trace part (name, calls, total ns, average ns, min ns, max ns):"
  stats "$tr"
} >> "$out" || exit 1
