#!/bin/bash
# Routes planned on the device (tools/batch_routes.py), 1 024 scenes of 64 with a street grid of 100 nodes each: (a) NO routes set --
# restart_device() and run(50) per tick on this build against the parent commit's build, alternated process by process in three
# rounds and in both orders (PARENT_LIB names the parent's libsfm_hip.so; skipped without it): the same kernels are launched, so the
# readings must lie inside the spread of the parent's own rounds; (b) plan_routes_device() with one routed row per scene and with
# every row routed, beside the host path a caller has without it (download, nx.astar_path per agent, set_modes again), alternated in
# three rounds; (c) the plan kernel's own duration from a kernel trace of 50 + 50 plans, a run of its own.  Each step under its own
# time limit, chained with &&.
# Output: OUT_DIR/r23_batch_routes.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/trace; OUT_DIR defaults to
# build/batch_routes (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_routes.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_routes}
out=$dir/r23_batch_routes.txt
err=$dir/stderr.log
mkdir -p "$dir/trace"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
k = [r for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)) for r in csv.DictReader(open(f))]
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
d = [dur(r) for r in k if "sfm_batch_plan_routes_kernel" in r["Kernel_Name"]]
for name, part in (("one routed row per scene", d[:50]), ("every row routed", d[-50:])):
    part = sorted(part)
    if part:
        print(f"# sfm_batch_plan_routes_kernel, {name}: {len(part)} launches, median {part[len(part) // 2]} ns, min {part[0]} ns, max {part[-1]} ns")
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (a) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (a) no routes set: the parent's build and this build, alternated process by process, both orders (per round: us per restart_device() call of 50, us per tick of run(50))"
  echo "build         B   N_b round us/restart_dev    us/tick"
  for r in 1 2; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_routes.py --part run --label parent &&
    timeout -k 10 240 python3 tools/batch_routes.py --part run --label this &&
    timeout -k 10 240 python3 tools/batch_routes.py --part run --label this &&
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_routes.py --part run --label parent || return 1
  done
}
trace() {
  echo "# (c) kernel trace of 50 plan_routes_device() calls with one routed row per scene and 50 with every row routed"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$dir/trace" -o rt -- \
      python3 tools/batch_routes.py --part trace && stats "$dir/trace"
}
echo "# tools/batch_routes.sh: routes planned on the device (sfm_batch_set_routes)" > "$out"
ab >> "$out" 2>> "$err" &&
timeout -k 10 400 python3 tools/batch_routes.py --part plan >> "$out" 2>> "$err" &&
trace >> "$out" 2>> "$err" || exit 1
