#!/bin/bash
# Vehicle episodes and vehicle respawns on a batch (tools/batch_vehicle_episodes.py), 1 024 scenes of 64 with 4 vehicles: (a) what
# existed before, with vehicle episodes never set -- run(50) per tick, end_step(), restart_device(), observe_vehicles() -- on this build
# against the parent commit's build, alternated process by process in both orders in three rounds (PARENT_LIB names the parent's
# libsfm_hip.so; skipped without it): this build's median must lie inside the parent's own min-max span; (b) the new calls beside
# end_step(), observe_vehicles(), one tick and the torch sequence of examples/batch_av_loop.py, alternated in three rounds; (c) the
# two kernels' own durations from a kernel trace, a run of its own.  Each step under its own time limit, chained with &&.
# Output: OUT_DIR/r27_batch_vehicle_episodes.txt (copy to profiles/ to keep it) and the trace under OUT_DIR/trace; OUT_DIR defaults to
# build/batch_vehicle_episodes (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_vehicle_episodes.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_vehicle_episodes}
out=$dir/r27_batch_vehicle_episodes.txt
err=$dir/stderr.log
mkdir -p "$dir/trace"
cd "$root" || exit 1
stats() {
  python3 - "$1" <<'PY'
import csv, glob, sys
k = [r for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)) for r in csv.DictReader(open(f))]
k.sort(key=lambda r: int(r["Start_Timestamp"]))
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
for name in ("sfm_batch_vehicle_episode_kernel", "sfm_batch_vehicle_respawn_kernel"):
    d = [dur(r) for r in k if name in r["Kernel_Name"]]
    half = len(d) // 2 if name.endswith("episode_kernel") else len(d)     # in launch order: one agent per scene, then every vehicle
    for what, part in (("first half" if half < len(d) else "all", sorted(d[:half])), ("second half", sorted(d[half:]))):
        if part:
            print(f"# {name}, {what}: {len(part)} launches, median {part[len(part) // 2]} ns, min {part[0]} ns, max {part[-1]} ns")
PY
}
spans() {
  python3 - "$1" <<'PY'
import statistics, sys
got = {}
for line in open(sys.argv[1]):
    p = line.split()
    if len(p) >= 4 and p[0] in ("parent", "this") and p[-2].isdigit():
        got.setdefault((" ".join(p[1:-2]), p[0]), []).append(float(p[-1]))
print("# (a) spans: form, the parent's min .. max, this build's median, inside?")
for form in dict.fromkeys(f for f, _ in got):
    pa, th = got.get((form, "parent"), []), got.get((form, "this"), [])
    if pa and th:
        m = statistics.median(th)
        print(f"# {form:<32} parent {min(pa):8.2f} .. {max(pa):8.2f} (median {statistics.median(pa):8.2f})   this {min(th):8.2f} .. {max(th):8.2f} "
              f"median {m:8.2f}   {'inside' if min(pa) <= m <= max(pa) else 'OUTSIDE'}")
PY
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (a) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (a) vehicle episodes never set: the parent's build and this build, alternated process by process in both orders (us per call, or per tick)"
  echo "build    form                             round         us"
  for r in 1 2 3; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 200 python3 tools/batch_vehicle_episodes.py --part paths --label parent &&
    timeout -k 10 200 python3 tools/batch_vehicle_episodes.py --part paths --label this &&
    timeout -k 10 200 python3 tools/batch_vehicle_episodes.py --part paths --label this &&
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 200 python3 tools/batch_vehicle_episodes.py --part paths --label parent || return 1
  done
}
trace() {
  echo "# (c) kernel trace of 50 end_vehicle_step() calls with one agent per scene, 50 with every vehicle an agent, 50 respawns of 1/8 of the vehicles"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$dir/trace" -o ve -- \
      python3 tools/batch_vehicle_episodes.py --part trace && stats "$dir/trace"
}
echo "# tools/batch_vehicle_episodes.sh: vehicle episodes and vehicle respawns on a batch (sfm_batch_end_vehicle_step, sfm_batch_respawn_vehicles_device)" > "$out"
ab >> "$out" 2>> "$err" && spans "$out" >> "$out.spans" && cat "$out.spans" >> "$out" && rm -f "$out.spans" &&
timeout -k 10 400 python3 tools/batch_vehicle_episodes.py --part vehicles >> "$out" 2>> "$err" &&
trace >> "$out" 2>> "$err" || exit 1
