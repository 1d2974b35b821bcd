"""Vehicle tracks on a batch (sfm_batch_set_vehicle_tracks): B = 1024 scenes of 64, all five forces, 4 device-side vehicles per
scene, timed with every vehicle tracked, free-running, and against the step-wise path a caller had before.
  --part free    `rounds` rounds of one run(ticks) call, no tracks -- run once per library build (SFM_LIB_PATH names another
                 build) and alternated by tools/batch_tracks.sh: (a) this build against its parent
  --part time    forms alternated in `rounds` rounds, each on a fresh upload: (f) free-running; (t) every vehicle tracked
                 (scenarios.make_track_plan over the call); then once (c) the step-wise path for the same traffic: per tick
                 place_tracked on the host, sfm_batch_set_dynamic_obstacles, run(1) -- `step_ticks` ticks of it
  --part trace   the tracks alone: 3 warm-up + `ticks` ticks -- for rocprofv3 --kernel-trace: ticks + 3 launches of the tick
                 kernel expected, nothing else between the first and the last
Times are host wall clock around one run(ticks) call after a 3-tick warm-up, closed by a device synchronisation."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from carla_social_force_model_amd import scenarios  # noqa: E402
from carla_social_force_model_amd._lib import fptr, iptr  # noqa: E402
from carla_social_force_model_amd.batch import SfmBatch, pack_boxes, pack_scenes  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402

POOL = 32
DT = 0.05


def _sync():
    import torch
    torch.cuda.synchronize()


class _Setup:
    def __init__(self, B, ticks, tracks=True):
        self.B = B
        pool = []
        for k in range(POOL):
            sc = vars(scenarios.make_scenario(64, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0)))
            pool.append((sc, scenarios.make_track_plan(sc, 7300 + k, ticks + 3, dt=DT)))
        self.scenes = [pool[k % POOL][0] for k in range(B)]
        self.tracks = [pool[k % POOL][1] for k in range(B)]
        self.boxes = pack_boxes(self.scenes)
        self.packed_tracks = None
        if tracks:
            from carla_social_force_model_amd.batch import pack_tracks
            self.packed_tracks = pack_tracks(self.tracks, self.boxes[0])
        self.batch = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)

    def fresh(self, tracked):
        b = self.batch
        b.upload(self.scenes, device_vehicles=True)
        if tracked:
            b.set_vehicle_tracks(self.packed_tracks)
        return b


def _time(b, ticks):
    b.run(3)
    _sync()
    t0 = time.perf_counter()
    b.run(ticks)
    _sync()
    return (time.perf_counter() - t0) / ticks


def _stepwise(s, ticks):
    """The traffic of form (t) without tracks on the device: every tick the host twin places every scene's vehicles, packs
    their rings and sends them with sfm_batch_set_dynamic_obstacles, then runs one tick."""
    b = s.batch
    b.upload(s.scenes)
    scenes = [dict(sc) for sc in s.scenes[:POOL]]                  # (the pool's 32 distinct scenes are placed once per tick each)
    _sync()
    t0 = time.perf_counter()
    for t in range(ticks):
        for k, sc in enumerate(scenes):
            scenarios.place_tracked(sc, s.tracks[k], t)
        dy = pack_scenes([scenes[k % POOL] for k in range(s.B)])["dynamic"]
        b._check(b._lib.sfm_batch_set_dynamic_obstacles(b._b, *(iptr(a) for a in dy[:2]), *(fptr(a) for a in dy[2:])),
                 "sfm_batch_set_dynamic_obstacles")
        b.run(1)
    _sync()
    return (time.perf_counter() - t0) / ticks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("free", "time", "trace"), default="time")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-ticks", type=int, default=5)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    B = 1024
    s = _Setup(B, args.ticks, tracks=args.part != "free")
    row = lambda f, r, t: print(f"{f:<8} {B:>6} {64:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
    try:
        if args.part == "free":
            print(f"# {args.label}: run({args.ticks}) with free-running vehicles, no tracks "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            b = s.fresh(False)
            for r in range(args.rounds):
                row(args.label, r, _time(b, args.ticks))
        elif args.part == "time":
            print(f"# vehicle tracks: B = {B} scenes of 64, all five forces, 4 device-side vehicles per scene; {args.ticks} ticks per "
                  f"call, forms alternated in {args.rounds} rounds on fresh uploads: (f) free-running, (t) every vehicle tracked")
            print(f"{'form':<8} {'B':>6} {'N_b':>5} {'round':>5} {'us/tick':>10} {'scene-ticks/s':>14}")
            for r in range(args.rounds):
                for f in "ft":
                    b = s.fresh(f == "t")
                    row(f, r, _time(b, args.ticks))
            tau, present = b.vehicle_tracks()
            print(f"# (t) after {tau} ticks: {int(sum(p.sum() for p in present))} of {4 * B} vehicles present")
            assert all(np.isfinite(v).all() for _, v in b.state())
            t = _stepwise(s, args.step_ticks)
            print(f"# (c) step-wise, the same traffic without tracks: per tick place_tracked on the host, pack, "
                  f"sfm_batch_set_dynamic_obstacles, run(1); {args.step_ticks} ticks")
            row("c", 0, t)
        else:
            b = s.fresh(True)
            t = _time(b, args.ticks)
            print(f"# trace: B = {B}, N_b = 64, all five forces, 4 tracked device-side vehicles per scene: 3 warm-up + {args.ticks} timed "
                  f"ticks = {args.ticks + 3} launches of sfm_batch_tick_kernel expected; {t * 1e6:.1f} us per tick (wall clock, under "
                  f"the tracer)")
    finally:
        s.batch.close()


if __name__ == "__main__":
    main()
