"""Spawn schedules on a batch (sfm_batch_set_spawn_schedule): B = 1024 scenes of 64, all five forces, 4 device-side vehicles per
scene and modes (the configuration of tools/batch_modes.py), timed with and without a schedule and against the step-wise path.
  --part modes   `rounds` rounds of one run(ticks) call, modes and no schedule -- run once per library build (SFM_LIB_PATH names
                 another build) and alternated by tools/batch_spawns.sh: (a) this build against its parent
  --part time    forms alternated in `rounds` rounds, each on a fresh upload: (m) modes, no schedule; (s) the same with a schedule
                 (a quarter of the rows arriving over the `ticks` ticks: scenarios.make_spawn_plan); then once (c) the step-wise
                 path for the same flow: per tick download the state, place the rows that are due on the host, upload + set_modes,
                 run(1) -- `step_ticks` ticks of it
  --part trace   the schedule alone: 3 warm-up + `ticks` ticks -- for rocprofv3 --kernel-trace: ticks + 3 launches of the tick
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
from carla_social_force_model_amd.batch import SfmBatch, pack_scenes  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402
from carla_social_force_model_amd.spawner import births  # noqa: E402

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
            # the clock the schedule is set on is 3 warm-up ticks ahead of sim_time0
            pool.append((sc, plan, lambda t0, sc=sc, k=k: scenarios.make_spawn_plan(sc, 7200 + k, dt=DT, t0=t0 + 3 * DT, present=0.75,
                                                                                   horizon=ticks * DT)))
        self.scenes = [pool[k % POOL][0] for k in range(B)]
        self.plans = [pool[k % POOL][1] for k in range(B)]
        self.t0 = [float(k % 5) for k in range(B)]
        self.scheds = [pool[k % POOL][2](self.t0[k]) for k in range(B)]
        self.packed = pack_scenes(self.scenes)
        self.batch = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)

    def fresh(self, spawns):
        b = self.batch
        b.upload(self.scenes, device_vehicles=True)
        b.set_modes(self.plans, sim_time0=self.t0, scenes=self.scenes)
        if spawns:
            b.set_spawns(self.scheds)
        return b


def _time(b, ticks):
    b.run(3)
    _sync()
    t0 = time.perf_counter()
    b.run(ticks)
    _sync()
    return (time.perf_counter() - t0) / ticks


def _stepwise(s, ticks):
    """The flow of form (s) without a schedule on the device: the host keeps who is born, and every tick downloads the state, puts
    the rows that are due at their spawn state, uploads, sets the modes again (upload resets them) and runs one tick."""
    b, B = s.batch, s.B
    b.upload(s.scenes, device_vehicles=True)
    b.set_modes(s.plans, sim_time0=s.t0, scenes=s.scenes)
    scenes = [dict(sc) for sc in s.scenes]
    born = [np.zeros(64, bool) for _ in range(B)]
    _sync()
    t0 = time.perf_counter()
    for t in range(ticks):
        state, modes, clocks = b.state(), b.modes(), b.clocks()
        plans = []
        for k in range(B):
            loc, vel = state[k]
            new = births(born[k], s.scheds[k]["spawn_time"], s.scheds[k]["chain"], clocks[k]) & ~born[k]
            loc[new], vel[new] = s.scenes[k]["loc"][new], s.scenes[k]["vel"][new]
            born[k] |= new
            scenes[k]["loc"], scenes[k]["vel"] = loc, vel
            plan = dict(s.plans[k])
            m, tg, cur = modes[k]
            plan["mode"], plan["target_speed"] = np.where(m > 4, 0, m), tg
            plan["queues"] = [q[c:] for q, c in zip(s.plans[k]["queues"], cur)]
            plans.append(plan)
        b.upload(scenes, device_vehicles=True)
        b.set_modes(plans, sim_time0=clocks, scenes=scenes)
        b.run(1)
    _sync()
    return (time.perf_counter() - t0) / ticks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("modes", "time", "trace"), default="time")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-ticks", type=int, default=5)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    B = 1024
    s = _Setup(B, args.ticks)
    row = lambda f, r, t: print(f"{f:<8} {B:>6} {64:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
    try:
        if args.part == "modes":
            print(f"# {args.label}: run({args.ticks}) with modes, no schedule ({os.path.basename(os.environ.get('SFM_LIB_PATH', '')) and 'the build named by SFM_LIB_PATH' or 'the in-tree build'})")
            b = s.fresh(False)
            for r in range(args.rounds):
                row(args.label, r, _time(b, args.ticks))
        elif args.part == "time":
            print(f"# spawn schedule: B = {B} scenes of 64, all five forces, 4 device-side vehicles and modes per scene; {args.ticks} ticks "
                  f"per call, forms alternated in {args.rounds} rounds on fresh uploads: (m) no schedule, (s) a schedule, a quarter of "
                  f"the rows arriving over the call")
            print(f"{'form':<8} {'B':>6} {'N_b':>5} {'round':>5} {'us/tick':>10} {'scene-ticks/s':>14}")
            for r in range(args.rounds):
                for f in "ms":
                    b = s.fresh(f == "s")
                    row(f, r, _time(b, args.ticks))
                    if f == "s":
                        born = np.concatenate([x for x, _ in b.spawns()])
                        when = np.concatenate([x for _, x in b.spawns()])
            late = int((when[born] > np.repeat(np.float32(s.t0), 64)[born] + np.float32(3 * DT - 1e-4)).sum())
            print(f"# (s) after {args.ticks + 3} ticks: {int(born.sum())} of {born.size} rows born, {late} of them during the timed call")
            assert all(np.isfinite(v).all() for _, v in b.state())
            t = _stepwise(s, args.step_ticks)
            print(f"# (c) step-wise, the same flow without a schedule: per tick state() + modes() + clocks(), rows placed on the host, "
                  f"upload() + set_modes(), run(1); {args.step_ticks} ticks")
            row("c", 0, t)
        else:
            b = s.fresh(True)
            t = _time(b, args.ticks)
            print(f"# trace: B = {B}, N_b = 64, all five forces, 4 device-side vehicles, modes and a spawn schedule per scene: 3 warm-up + "
                  f"{args.ticks} timed ticks = {args.ticks + 3} launches of sfm_batch_tick_kernel<.., .., true, true> expected; "
                  f"{t * 1e6:.1f} us per tick (wall clock, under the tracer)")
    finally:
        s.batch.close()


if __name__ == "__main__":
    main()
