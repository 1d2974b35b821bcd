"""Force records on a batch (sfm_batch_tick_forces, sfm_batch_run_recorded_forces): B = 1024 scenes of 64, all five forces (2 borders,
2 static obstacles, 4 device-side vehicles per scene), timed in alternating rounds on one batch of each form.
  --part time    `rounds` rounds of one call of `ticks` ticks per form:  (r) run,  (f) run_recorded (every tick),  (t) run_recorded_forces
                 with the total only,  (a) run_recorded_forces with all six forces,  (s) `ticks` step-wise tick_forces(integrate=True)
  --part trace   run_recorded_forces(ticks) with all six -- for rocprofv3 --kernel-trace: `ticks` launches of the EXT kernel
                 expected, and no copy between the first and the last
  --part plain   (r) alone, for an A/B of library builds (SFM_LIB_PATH)
Times are host wall clock around one call after a 3-tick warm-up, closed by a device synchronisation (the recorded forms return
with their copies done)."""
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
FORMS = {"r": "run", "f": "run_recorded", "t": "run_recorded_forces total", "a": "run_recorded_forces all six",
         "s": "tick_forces(integrate) x ticks"}


def _sync():
    import torch
    torch.cuda.synchronize()


def _batch(B):
    pool = [vars(scenarios.make_scenario(64, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0)))
            for k in range(POOL)]
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), 0.05, B=B)
    b.upload([pool[k % POOL] for k in range(B)], device_vehicles=True)
    return b


def _call(b, form, ticks):
    if form == "r":
        b.run(ticks)
    elif form == "f":
        b.run_recorded(ticks)
    elif form == "t":
        b.run_recorded_forces(ticks, forces="total")
    elif form == "a":
        b.run_recorded_forces(ticks)
    else:
        for _ in range(ticks):
            b.tick_forces(integrate=True)


def _time(b, form, ticks):
    b.run(3)
    _sync()
    t0 = time.perf_counter()
    _call(b, form, ticks)
    _sync()
    return (time.perf_counter() - t0) / ticks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("time", "trace", "plain"), default="time")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    B = 1024
    b = _batch(B)
    try:
        if args.part == "time":
            print(f"# force records: B = {B} scenes of 64, all five forces, 2 borders, 2 static, 4 device-side vehicles per scene; "
                  f"{args.ticks} ticks per call, forms alternated in {args.rounds} rounds on one batch: " +
                  "; ".join(f"({k}) {v}" for k, v in FORMS.items()))
            print(f"{'form':<6} {'B':>6} {'N_b':>5} {'round':>5} {'us/tick':>10} {'scene-ticks/s':>14}")
            for r in range(args.rounds):
                for f in FORMS:
                    t = _time(b, f, args.ticks)
                    print(f"{f:<6} {B:>6} {64:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
            assert all(np.isfinite(v).all() for _, v in b.state())
        elif args.part == "plain":
            for r in range(args.rounds):
                t = _time(b, "r", args.ticks)
                print(f"plain run({args.ticks}) round {r}: {t * 1e6:.1f} us per tick", flush=True)
        else:
            t = _time(b, "a", args.ticks)
            print(f"# trace: B = {B}, N_b = 64, all five forces and 4 device-side vehicles per scene: 3 warm-up + {args.ticks} "
                  f"recorded ticks = {args.ticks} launches of sfm_batch_tick_kernel<false, true, false> and 3 of <false, false, "
                  f"false> expected; {t * 1e6:.1f} us per tick (wall clock, under the tracer)")
    finally:
        b.close()


if __name__ == "__main__":
    main()
