"""Pedestrian modes on a batch (sfm_batch_set_mode_fsm): B = 1024 scenes of 64, all five forces, 4 device-side vehicles per scene,
with and without modes (queues of 3 waypoints, idle and reckless pedestrians: scenarios.make_mode_plan), timed in alternating
rounds against the same batch.
  --part time    `rounds` rounds of one run(ticks) call per form: (a) no modes, (m) modes
  --part trace   modes alone: set_modes, 3 warm-up + `ticks` ticks -- for rocprofv3 --kernel-trace: ticks + 3 launches of the MODES
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
from carla_social_force_model_amd.batch import SfmBatch  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402

POOL = 32


def _sync():
    import torch
    torch.cuda.synchronize()


def _batch(B, modes):
    pool = []
    for k in range(POOL):
        sc = vars(scenarios.make_scenario(64, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0)))
        plan, _ = scenarios.make_mode_plan(sc, 7100 + k)
        pool.append((sc, plan))
    scenes = [pool[k % POOL][0] for k in range(B)]
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), 0.05, B=B)
    b.upload(scenes, device_vehicles=True)
    if modes:
        b.set_modes([pool[k % POOL][1] for k in range(B)], sim_time0=[float(k % 5) for k in range(B)], scenes=scenes)
    return b


def _time(b, ticks):
    b.run(3)
    _sync()
    t0 = time.perf_counter()
    b.run(ticks)
    _sync()
    return (time.perf_counter() - t0) / ticks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("time", "trace"), default="time")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    B = 1024
    if args.part == "time":
        print(f"# modes: B = {B} scenes of 64, all five forces, 4 device-side vehicles per scene; {args.ticks} ticks per call, forms "
              f"alternated in {args.rounds} rounds: (a) no modes, (m) modes (queues of 3, idle and reckless pedestrians)")
        print(f"{'form':<6} {'B':>6} {'N_b':>5} {'round':>5} {'us/tick':>10} {'scene-ticks/s':>14}")
        batches = {"a": _batch(B, False), "m": _batch(B, True)}
        try:
            for r in range(args.rounds):
                for f in "am":
                    t = _time(batches[f], args.ticks)
                    print(f"{f:<6} {B:>6} {64:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
            mode = np.concatenate([m for m, _, _ in batches["m"].modes()])
            counts = np.bincount(mode, minlength=256)
            print(f"# modes after {args.rounds * (args.ticks + 3)} ticks: idle {counts[0]}, walking {counts[1]}, crossing {counts[2]}, "
                  f"road-to-sidewalk {counts[3]}, checking {counts[4]}, despawned {counts[255]}")
            assert all(np.isfinite(v).all() for f in "am" for _, v in batches[f].state())
        finally:
            for b in batches.values():
                b.close()
    else:
        b = _batch(B, True)
        try:
            t = _time(b, args.ticks)
        finally:
            b.close()
        print(f"# trace: B = {B}, N_b = 64, all five forces, 4 device-side vehicles and modes per scene: 3 warm-up + {args.ticks} "
              f"timed ticks = {args.ticks + 3} launches of sfm_batch_tick_kernel<.., .., true> expected; {t * 1e6:.1f} us per tick "
              f"(wall clock, under the tracer)")


if __name__ == "__main__":
    main()
