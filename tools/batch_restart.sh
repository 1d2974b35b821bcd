#!/bin/bash
# Snapshot and restart on a batch (tools/batch_restart.py): (a) run(50) on this build against the parent commit's build, alternated
# process by process (PARENT_LIB names the parent's libsfm_hip.so; skipped without it), (b) snapshot, restart of 1 scene / 10 % /
# all scenes and the upload + set_* path through the packers (--part time), and a kernel + memory-copy trace of a run with a
# restart every 10 ticks: each step under its own time limit, chained with &&.
# Output: OUT_DIR/r13_batch_restart.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/restart_trace; OUT_DIR defaults
# to build/batch_restart (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_restart.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_restart}
out=$dir/r13_batch_restart.txt
tr=$dir/restart_trace
err=$dir/stderr.log
mkdir -p "$dir" "$tr"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
for kind in ("kernel_stats", "memory_copy_stats"):
    files = sorted(glob.glob(sys.argv[1] + f"/**/*{kind}.csv", recursive=True))
    if kind == "memory_copy_stats":
        print("# memory copies over the whole process (uploads, set-up, the snapshot):" if files else "# no memory copies traced")
    for f in files:
        for r in csv.DictReader(open(f)):
            print(f"{r['Name'][:60]:<60} {r['Calls']:>6} {r['TotalDurationNs']:>12} {float(r['AverageNs']):>10.0f} {r['MinNs']:>8} {r['MaxNs']:>8}")
kt = sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True))
mt = sorted(glob.glob(sys.argv[1] + "/**/*memory_copy_trace.csv", recursive=True))
k = [r for f in kt for r in csv.DictReader(open(f))]
m = [r for f in mt for r in csv.DictReader(open(f))]
ticks = [r for r in k if "sfm_batch_tick_kernel" in r["Kernel_Name"]]
restarts = [r for r in k if "sfm_batch_restart_kernel" in r["Kernel_Name"]]
if ticks and restarts:
    # from the first restart on (the snapshot's copies come before it) to the last tick launch
    t0, t1 = min(int(r["Start_Timestamp"]) for r in restarts), max(int(r["End_Timestamp"]) for r in ticks)
    inside = lambda r: t0 <= int(r["Start_Timestamp"]) <= t1
    first = min(int(r["Start_Timestamp"]) for r in ticks)
    copies = [r for r in m if first <= int(r["Start_Timestamp"]) <= t1]
    kinds = sorted({r.get("Direction", "?") for r in copies})
    print(f"# {len(ticks)} tick launches, {len(restarts)} restart launches; between the first tick launch and the last: "
          f"{len(copies)} memory copies ({', '.join(kinds) or 'none'}; the snapshot's device-to-device copies and one list of "
          f"scenes per restart), {sum(1 for r in k if first <= int(r['Start_Timestamp']) <= t1 and r not in ticks and r not in restarts)} "
          f"other kernel launches; from the first restart on: {sum(map(inside, m))} memory copies")
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (a) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (a) run(50): the parent's build and this build, alternated process by process (us/tick per round of run(50))"
  echo "build         B   N_b round    us/tick  scene-ticks/s"
  for r in 1 2 3; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_restart.py --part run --label parent &&
    timeout -k 10 240 python3 tools/batch_restart.py --part run --label this || return 1
  done
}
echo "# tools/batch_restart.sh: snapshot and restart on a batch (sfm_batch_snapshot, sfm_batch_restart)" > "$out"
ab >> "$out" 2>> "$err" &&
timeout -k 10 600 python3 tools/batch_restart.py --part time >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d "$tr" -o br -- \
    python3 tools/batch_restart.py --part trace --ticks 100 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace --memory-copy-trace --stats of the trace part (name, calls, total ns, average ns, min ns, max ns):"
  stats "$tr"
} >> "$out" || exit 1
