#!/bin/bash
# Episode ends and the restart by device mask on a batch (tools/batch_episodes.py): (a) end_step() beside observe() and one tick
# launch, (c) restart_device() against restart(mask) with 1/8 of the scenes chosen, alternated in three rounds of 50 calls (--part
# ep); (b) one loop step of examples/batch_rl_loop.py against one of examples/batch_rl_loop_device.py at 1 024 scenes and 4 ticks per
# step, alternated in three rounds (--part loop), and a kernel + memory-copy trace of 50 steps of each loop: launches and copies per
# step (copies: what the memory-copy trace lists plus the launches of the runtime's own copy kernel, which carries small copies);
# (d) run(50) of the batch without episodes on this build against the parent commit's build, alternated process by process
# (PARENT_LIB names the parent's libsfm_hip.so; skipped without it).  Each step under its own time limit, chained with &&.
# Output: OUT_DIR/r16_batch_episodes.txt (copy to profiles/ to keep it) and the traces under OUT_DIR/trace_host and
# OUT_DIR/trace_device; OUT_DIR defaults to build/batch_episodes (not tracked).  Standard error goes to OUT_DIR/stderr.log.
#   [PARENT_LIB=path/to/parent/libsfm_hip.so] bash tools/batch_episodes.sh [OUT_DIR]
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$root/build/batch_episodes}
out=$dir/r16_batch_episodes.txt
err=$dir/stderr.log
steps=50
mkdir -p "$dir/trace_host" "$dir/trace_device"
cd "$root" || exit 1
stats() {
  python3 - "$1" "$steps" <<'PY'
import csv, glob, sys
steps = int(sys.argv[2])
k = [r for f in sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)) for r in csv.DictReader(open(f))]
m = [r for f in sorted(glob.glob(sys.argv[1] + "/**/*memory_copy_trace.csv", recursive=True)) for r in csv.DictReader(open(f))]
dur = lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
ours = ("sfm_batch_tick_kernel", "sfm_batch_observe_kernel", "sfm_batch_episode_kernel", "sfm_batch_restart_kernel")
for name in ours:
    d = sorted(dur(r) for r in k if name in r["Kernel_Name"])
    if d:
        print(f"# {name}: {len(d)} launches, median {d[len(d) // 2]} ns, min {d[0]} ns, max {d[-1]} ns")
obs = [r for r in k if "sfm_batch_observe_kernel" in r["Kernel_Name"]]
last = [r for r in k if any(n in r["Kernel_Name"] for n in ours)]
if obs and last:
    # the loop: from the first observe launch to the end of the library's last launch (set-up, uploads and the snapshot come before)
    t0, t1 = min(int(r["Start_Timestamp"]) for r in obs), max(int(r["End_Timestamp"]) for r in last)
    inside = lambda r: t0 <= int(r["Start_Timestamp"]) <= t1
    lib = [r for r in k if inside(r) and any(n in r["Kernel_Name"] for n in ours)]
    # the HIP runtime makes small copies (a mask to the host, a list to the device, .item()) with a kernel of its own, which the
    # memory-copy trace does not list: they are counted as copies here, by name
    by_kernel = [r for r in k if inside(r) and "__amd_rocclr_copy" in r["Kernel_Name"]]
    other = [r for r in k if inside(r) and not any(n in r["Kernel_Name"] for n in ours) and "__amd_rocclr_copy" not in r["Kernel_Name"]]
    copies = [r for r in m if inside(r)]
    kinds = {}
    for r in copies:
        kinds[r.get("Direction", "?")] = kinds.get(r.get("Direction", "?"), 0) + 1
    print(f"# inside the loop ({steps} steps): {len(lib)} launches of the library's kernels ({len(lib) / steps:.2f} per step), "
          f"{len(other)} other launches (torch: the policy, the tally; {len(other) / steps:.2f} per step), "
          f"{len(copies)} traced memory copies{''.join(f'; {v} {n}' for n, v in sorted(kinds.items()))} and {len(by_kernel)} copies "
          f"made by the runtime's copy kernel (__amd_rocclr_copy*): {(len(copies) + len(by_kernel)) / steps:.2f} copies per step")
PY
}
trace() {
  timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d "$dir/trace_$1" -o be -- \
      python3 tools/batch_episodes.py --part trace --example "$1" --steps $steps && stats "$dir/trace_$1"
}
ab() {
  if [ -z "$PARENT_LIB" ]; then echo "# (d) skipped: PARENT_LIB not set"; return 0; fi
  echo "# (d) run(50) without episodes: the parent's build and this build, alternated process by process (us/tick per round of run(50))"
  echo "build         B   N_b round    us/tick  scene-ticks/s"
  for r in 1 2 3; do
    SFM_LIB_PATH=$PARENT_LIB timeout -k 10 240 python3 tools/batch_episodes.py --part run --label parent &&
    timeout -k 10 240 python3 tools/batch_episodes.py --part run --label this || return 1
  done
}
echo "# tools/batch_episodes.sh: episode ends and the restart by device mask on a batch (sfm_batch_set_episodes, sfm_batch_end_step, sfm_batch_restart_device)" > "$out"
timeout -k 10 300 python3 tools/batch_episodes.py --part ep >> "$out" 2>> "$err" &&
timeout -k 10 300 python3 tools/batch_episodes.py --part loop >> "$out" 2>> "$err" &&
ab >> "$out" 2>> "$err" &&
trace host >> "$out" 2>> "$err" &&
trace device >> "$out" 2>> "$err" || exit 1
