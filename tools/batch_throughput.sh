#!/bin/bash
# Batched scenes against one handle per scene (tools/batch_throughput.py), and the kernel trace of a batch run: each step under its
# own time limit, chained with &&.  Output: OUT_DIR/r05_batch_throughput.txt (copy to profiles/ to keep it) and the trace under
# OUT_DIR/batch_trace; OUT_DIR defaults to build/batch_throughput (not tracked).
#   bash tools/batch_throughput.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_throughput}
out=$dir/r05_batch_throughput.txt
tr=$dir/batch_trace
mkdir -p "$dir" "$tr"
cd "$root" || exit 1
echo "# tools/batch_throughput.sh: batched scenes (sfm_batch_tick_kernel, one launch per tick) vs one SfmEngine handle per scene" > "$out"
timeout -k 10 900 python3 tools/batch_throughput.py --part batch >> "$out" 2>&1 &&
timeout -k 10 900 python3 tools/batch_throughput.py --part handles >> "$out" 2>&1 &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$tr" -o bt -- \
    python3 tools/batch_throughput.py --part trace --ticks 100 >> "$out" 2>&1 &&
{
  echo "# rocprofv3 --kernel-trace --stats of the trace part (kernel, calls, total ns, average ns, min ns, max ns):"
  python3 - "$tr" <<'PY'
import csv, glob, sys
for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_stats.csv", recursive=True)):
    for r in csv.DictReader(open(f)):
        print(f"{r['Name'][:60]:<60} {r['Calls']:>6} {r['TotalDurationNs']:>12} {float(r['AverageNs']):>10.0f} {r['MinNs']:>8} {r['MaxNs']:>8}")
PY
} >> "$out"
