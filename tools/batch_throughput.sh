#!/bin/bash
# Batched scenes against one handle per scene, waypoint streams and recorded runs (tools/batch_throughput.py), and kernel traces of
# a plain and a recorded batch run: each step under its own time limit, chained with &&.  Output: OUT_DIR/r06_batch_streams.txt
# (copy to profiles/ to keep it) and the traces under OUT_DIR/batch_trace*; OUT_DIR defaults to build/batch_throughput (not tracked).
# BASE_LIB=<path to another build's libsfm_hip.so> adds an A/B of plain run(50) rows, alternating that build and the in-tree one.
# Standard error of every step (runtime and profiler diagnostics) goes to OUT_DIR/stderr.log.
#   [BASE_LIB=...] bash tools/batch_throughput.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_throughput}
out=$dir/r06_batch_streams.txt
tr=$dir/batch_trace
trr=$dir/batch_trace_recorded
err=$dir/stderr.log
mkdir -p "$dir" "$tr" "$trr"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_stats.csv", recursive=True)):
    for r in csv.DictReader(open(f)):
        print(f"{r['Name'][:60]:<60} {r['Calls']:>6} {r['TotalDurationNs']:>12} {float(r['AverageNs']):>10.0f} {r['MinNs']:>8} {r['MaxNs']:>8}")
PY
}
ab() {
  [ -z "$BASE_LIB" ] && return 0
  base=$(cd "$(dirname "$BASE_LIB")" && pwd)/$(basename "$BASE_LIB")
  echo "# A/B of plain run(50): the build BASE_LIB names (loaded through SFM_LIB_PATH) and the in-tree build, alternated"
  for i in 1 2 3; do
    SFM_LIB_PATH=$base timeout -k 10 300 python3 tools/batch_throughput.py --part plain --rounds 2 2>> "$err" || return 1
    timeout -k 10 300 python3 tools/batch_throughput.py --part plain --rounds 2 2>> "$err" || return 1
  done
}
echo "# tools/batch_throughput.sh: batched scenes (sfm_batch_tick_kernel, one launch per tick) vs one SfmEngine handle per scene" > "$out"
timeout -k 10 900 python3 tools/batch_throughput.py --part batch >> "$out" 2>> "$err" &&
timeout -k 10 900 python3 tools/batch_throughput.py --part handles >> "$out" 2>> "$err" &&
timeout -k 10 600 python3 tools/batch_throughput.py --part streams >> "$out" 2>> "$err" &&
ab >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$tr" -o bt -- \
    python3 tools/batch_throughput.py --part trace --ticks 100 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace --stats of the trace part (kernel, calls, total ns, average ns, min ns, max ns):"
  stats "$tr"
} >> "$out" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$trr" -o btr -- \
    python3 tools/batch_throughput.py --part trace-recorded --ticks 100 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace --stats of the trace-recorded part (kernel, calls, total ns, average ns, min ns, max ns):"
  stats "$trr"
} >> "$out"
