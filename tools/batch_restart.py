"""Snapshot and restart on a batch (sfm_batch_snapshot, sfm_batch_restart): B = 1024 scenes of 64, all five forces, 4 tracked
device-side vehicles, modes and a spawn schedule per scene.
  --part run     `rounds` rounds of one run(ticks) call -- run once per library build (SFM_LIB_PATH names another build) and
                 alternated by tools/batch_restart.sh: this build against its parent (the tick kernel is the parent's)
  --part time    alternated in `rounds` rounds, `ticks` ticks between them: snapshot(); restart of 1 scene, of 10 % of the scenes
                 and of all scenes; and (u) the path a caller had before, for all scenes: upload, set_vehicle_tracks, set_modes and
                 set_spawns from the scene dicts, through the packers.  Medians at the end
  --part trace   3 warm-up ticks, snapshot(), then `ticks` / 10 times run(10) + restart(10 % of the scenes) -- for rocprofv3
                 --kernel-trace --memory-copy-trace: one sfm_batch_restart_kernel launch per restart, one sfm_batch_tick_kernel
                 launch per tick, and between them no copy but each restart's list of scenes
Times are host wall clock around the call, closed by a device synchronisation."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from carla_social_force_model_amd import scenarios  # noqa: E402
from carla_social_force_model_amd.batch import SfmBatch  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402

POOL = 32
DT = 0.05


def _sync():
    import torch
    torch.cuda.synchronize()


class _Setup:
    def __init__(self, B, ticks):
        self.B = B
        pool = []
        for k in range(POOL):
            sc = vars(scenarios.make_scenario(64, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0)))
            plan, _ = scenarios.make_mode_plan(sc, 7100 + k)
            sched = scenarios.make_spawn_plan(sc, 7200 + k, dt=DT, horizon=ticks * DT)
            pool.append((sc, plan, sched, scenarios.make_track_plan(sc, 7300 + k, ticks + 3, dt=DT)))
        self.scenes, self.plans, self.scheds, self.tracks = ([pool[k % POOL][q] for k in range(B)] for q in range(4))
        self.batch = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)

    def fresh(self):
        """The path a caller has without a snapshot: everything from the scene dicts, through the packers."""
        b = self.batch
        b.upload(self.scenes, device_vehicles=True)
        b.set_vehicle_tracks(self.tracks)
        b.set_modes(self.plans, scenes=self.scenes)
        b.set_spawns(self.scheds)
        return b


def _timed(fn):
    _sync()
    t0 = time.perf_counter()
    fn()
    _sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("run", "time", "trace"), default="time")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    B = 1024
    s = _Setup(B, args.ticks)
    tenth = np.arange(0, B, 10)
    what = f"B = {B} scenes of 64, all five forces, 4 tracked device-side vehicles, modes and a spawn schedule per scene"
    try:
        if args.part == "run":
            print(f"# {args.label}: run({args.ticks}), {what} "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            b = s.fresh()
            b.run(3)
            for r in range(args.rounds):
                t = _timed(lambda: b.run(args.ticks)) / args.ticks
                print(f"{args.label:<8} {B:>6} {64:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
        elif args.part == "time":
            print(f"# snapshot and restart: {what}; {args.ticks} ticks between the rounds")
            print(f"{'call':<14} {'scenes':>6} {'round':>5} {'us':>12}")
            forms = (("snapshot", B, lambda b: b.snapshot()), ("restart", 1, lambda b: b.restart([B // 2])),
                     ("restart", len(tenth), lambda b: b.restart(tenth)), ("restart", B, lambda b: b.restart()),
                     ("u: packers", B, lambda b: s.fresh()))
            got = {(n, c): [] for n, c, _ in forms}
            b = s.fresh()
            b.run(3)
            b.snapshot()
            b.restart([0])                                             # (the first masked restart allocates its list)
            for r in range(args.rounds):
                for name, count, fn in forms:
                    b.run(args.ticks)
                    t = _timed(lambda: fn(b))
                    if name.startswith("u"):                           # (the upload dropped the snapshot)
                        b.snapshot()
                    got[(name, count)].append(t)
                    print(f"{name:<14} {count:>6} {r:>5} {t * 1e6:>12.1f}", flush=True)
            print("# medians (us), and the packers' path over each")
            u = statistics.median(got[("u: packers", B)])
            for (name, count), ts in got.items():
                m = statistics.median(ts)
                print(f"{name:<14} {count:>6} {'med':>5} {m * 1e6:>12.1f} {u / m:>10.0f}x")
            assert all(np.isfinite(v).all() for _, v in b.state())
        else:
            b = s.fresh()
            b.run(3)
            b.snapshot()
            n = max(1, args.ticks // 10)
            t = _timed(lambda: [(b.run(10), b.restart(tenth)) for _ in range(n)])
            print(f"# trace: {what}: 3 warm-up ticks, snapshot(), then {n} x (run(10), restart of {len(tenth)} scenes) = {10 * n + 3} "
                  f"launches of sfm_batch_tick_kernel and {n} of sfm_batch_restart_kernel expected; {t * 1e6 / n:.1f} us per block "
                  f"of 10 ticks and a restart (wall clock, under the tracer)")
    finally:
        s.batch.close()


if __name__ == "__main__":
    main()
