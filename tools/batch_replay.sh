#!/bin/bash
# Observed tracks on a batch (tools/batch_replay.py): (a) run_observed per tick, run per tick, score(), scene_scores() and the path a
# caller had before (set_commands per tick, run_recorded, ADE in NumPy), alternated in three rounds of 50 (--part replay); (b) run(50)
# and restart_device() of the batch without observed tracks on this build against the parent commit's build, alternated process by
# process (PARENT_LIB names the parent's libsfm_hip.so; skipped without it); and a kernel trace of 50 frames of run_observed and 50 x
# score(): one sfm_batch_replay_kernel and one sfm_batch_score_kernel launch beside one tick.  Each step under its own time limit,
# chained with &&.
# Output: OUT_DIR/r20_batch_replay.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/replay_trace; OUT_DIR defaults to
# build/batch_replay (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_replay.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_replay}
out=$dir/r20_batch_replay.txt
tr=$dir/replay_trace
err=$dir/stderr.log
mkdir -p "$dir" "$tr"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
k = [r for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)) for r in csv.DictReader(open(f))]
k.sort(key=lambda r: int(r["Start_Timestamp"]))
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
def line(name, d):
    d = sorted(d)
    if d:
        print(f"# {name}: {len(d)} launches, median {d[len(d) // 2]} ns, min {d[0]} ns, max {d[-1]} ns")
ticks = [dur(r) for r in k if "sfm_batch_tick_kernel" in r["Kernel_Name"]]
line("sfm_batch_tick_kernel (warm-up launches left out)", ticks[3:])
line("sfm_batch_replay_kernel", [dur(r) for r in k if "sfm_batch_replay_kernel" in r["Kernel_Name"]])
line("sfm_batch_score_kernel", [dur(r) for r in k if "sfm_batch_score_kernel" in r["Kernel_Name"]])
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (b) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (b) the paths that existed, without observed tracks: the parent's build and this build, alternated process by process (us per call, per round of 50)"
  echo "build    call                             round    us/call"
  for r in 1 2 3; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_replay.py --part existing --label parent &&
    timeout -k 10 240 python3 tools/batch_replay.py --part existing --label this || return 1
  done
}
echo "# tools/batch_replay.sh: observed tracks on a batch (sfm_batch_set_observed, sfm_batch_run_observed, sfm_batch_score); 1 024 scenes of 64, every = 1, 50 frames" > "$out"
timeout -k 10 300 python3 tools/batch_replay.py --part replay >> "$out" 2>> "$err" &&
ab >> "$out" 2>> "$err" &&
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$tr" -o br -- \
    python3 tools/batch_replay.py --part trace --ticks 50 >> "$out" 2>> "$err" &&
{
  echo "# rocprofv3 --kernel-trace of the trace part:"
  stats "$tr"
} >> "$out" || exit 1
