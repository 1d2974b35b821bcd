#!/bin/bash
# Vehicle tracks on a batch (tools/batch_tracks.py): (a) run(50) with free-running vehicles and no tracks on this build against the parent
# commit's build, alternated process by process (PARENT_LIB names the parent's libsfm_hip.so; skipped without it), (b) the same
# batch with every vehicle tracked and (c) the step-wise path (--part time), and a kernel + memory-copy trace of the tracks alone: each
# step under its own time limit, chained with &&.
# Output: OUT_DIR/r12_batch_tracks.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/tracks_trace; OUT_DIR defaults
# to build/batch_tracks (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_tracks.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_tracks}
out=$dir/r12_batch_tracks.txt
tr=$dir/tracks_trace
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
ticks = [r for r in k if "sfm_batch_tick_kernel" in r["Kernel_Name"]]
if ticks:
    t0, t1 = min(int(r["Start_Timestamp"]) for r in ticks), max(int(r["End_Timestamp"]) for r in ticks)
    inside = lambda r: t0 <= int(r["Start_Timestamp"]) <= t1
    print(f"# between the first and the last of the {len(ticks)} tick launches: {sum(map(inside, m))} memory copies, "
          f"{sum(1 for r in k if inside(r) and r not in ticks)} other kernel launches")
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (a) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (a) free-running vehicles, no tracks: the parent's build and this build, alternated process by process (us/tick per round of run(50))"
  echo "form          B   N_b round    us/tick  scene-ticks/s"
  for r in 1 2 3; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_tracks.py --part free --label parent &&
    timeout -k 10 240 python3 tools/batch_tracks.py --part free --label this || return 1
  done
}
echo "# tools/batch_tracks.sh: vehicle tracks on a batch (sfm_batch_set_vehicle_tracks)" > "$out"
ab >> "$out" 2>> "$err" &&
timeout -k 10 900 python3 tools/batch_tracks.py --part time >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d "$tr" -o bt -- \
    python3 tools/batch_tracks.py --part trace --ticks 100 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace --memory-copy-trace --stats of the trace part (name, calls, total ns, average ns, min ns, max ns):"
  stats "$tr"
} >> "$out" || exit 1
