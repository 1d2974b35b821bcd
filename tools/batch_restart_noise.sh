#!/bin/bash
# Restart noise on a batch (tools/batch_restart_noise.py), 1 024 scenes of 64, every eighth chosen: (a) noise OFF -- restart_device()
# and run(50) per tick on this build against the parent commit's build, alternated process by process in three rounds (PARENT_LIB
# names the parent's libsfm_hip.so; skipped without it): the same kernels are launched, so the readings must lie inside the
# spread of the parent's own rounds; (b) noise ON -- restart_device() with noise off and on (tries 8, gaps 0.6 m / 0.3 m) beside the
# host path a caller had before (download, NumPy twin, upload, steering, observation, episodes and scan set again), alternated in
# three rounds; (c) the noise kernel's own duration from a kernel trace of 50 noisy restarts, a run of its own.  Each step under
# its own time limit, chained with &&.
# Output: OUT_DIR/r18_batch_restart_noise.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/trace; OUT_DIR defaults to
# build/batch_restart_noise (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_restart_noise.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_restart_noise}
out=$dir/r18_batch_restart_noise.txt
err=$dir/stderr.log
mkdir -p "$dir/trace"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
k = [r for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)) for r in csv.DictReader(open(f))]
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
for name in ("sfm_batch_restart_kernel", "sfm_batch_restart_noise_kernel"):
    d = sorted(dur(r) for r in k if name in r["Kernel_Name"])
    if d:
        print(f"# {name}: {len(d)} launches, median {d[len(d) // 2]} ns, min {d[0]} ns, max {d[-1]} ns")
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (a) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (a) noise off: the parent's build and this build, alternated process by process (per round: us per restart_device() call of 50, us per tick of run(50))"
  echo "build         B   N_b round us/restart_dev    us/tick"
  for r in 1 2 3; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_restart_noise.py --part run --label parent &&
    timeout -k 10 240 python3 tools/batch_restart_noise.py --part run --label this || return 1
  done
}
trace() {
  echo "# (c) kernel trace of 50 noisy restart_device() calls (and of the set-up's launches of the restart kernel)"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$dir/trace" -o rn -- \
      python3 tools/batch_restart_noise.py --part trace && stats "$dir/trace"
}
echo "# tools/batch_restart_noise.sh: restart noise on a batch (sfm_batch_set_restart_noise)" > "$out"
ab >> "$out" 2>> "$err" &&
timeout -k 10 400 python3 tools/batch_restart_noise.py --part noise >> "$out" 2>> "$err" &&
trace >> "$out" 2>> "$err" || exit 1
