"""Vehicle episodes and vehicle respawns on a batch (sfm_batch_end_vehicle_step, sfm_batch_respawn_vehicles_device): B = 1024 scenes
of 64, all five forces, 4 moving device-side vehicles per scene.
  --part paths      `rounds` rounds of `calls` calls of what existed before, with vehicle episodes never set: run(ticks) per tick,
                    end_step(), restart_device() of every eighth scene, observe_vehicles() -- run once per library build
                    (SFM_LIB_PATH names another build) and alternated by tools/batch_vehicle_episodes.sh: this build against its parent
  --part vehicles   alternated in `rounds` rounds (us per call, medians at the end): one tick, end_step() and observe_vehicles()
                    beside end_vehicle_step() with one agent vehicle per scene and with all 4 096 vehicles agents,
                    respawn_vehicles_device() of 1/8 of the vehicles, and the torch sequence of examples/batch_av_loop.py that
                    end_vehicle_step replaces (goal distance, clearance tests on slot 8, an age counter, the done mask) -- which
                    yields the pedestrian clearance of the sampled ring only, no vehicle and no wall gap
  --part trace      `calls` calls of end_vehicle_step() with one agent per scene, then with every vehicle an agent, then of the
                    respawn -- for rocprofv3 --kernel-trace --stats
Times are host wall clock around the calls, closed by a device synchronisation."""
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

POOL, DT, N_B, M_B, K, RANGE = 32, 0.05, 64, 4, 4, 12.0
RADII = dict(goal_radius=1.0, ped_radius=0.3, veh_radius=0.3, max_steps=0)


def _sync():
    import torch
    torch.cuda.synchronize()


def _timed(fn, calls):
    _sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    _sync()
    return (time.perf_counter() - t0) / calls


def _scenes(B):
    pool = [vars(scenarios.make_scenario(N_B, 7000 + k, n_borders=2, n_static=2, n_dynamic=M_B, border_len=(2.0, 2.0))) for k in range(POOL)]
    return [pool[k % POOL] for k in range(B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("paths", "vehicles", "trace"), default="vehicles")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    ap.add_argument("--scenes", type=int, default=1024)
    args = ap.parse_args()
    import torch
    B, calls = args.scenes, args.calls
    M = B * M_B
    what = f"B = {B} scenes of {N_B}, all five forces, {M_B} moving device-side vehicles per scene"
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        b.upload(_scenes(B), device_vehicles=True)
        b.set_episodes(0, **RADII)
        b.set_vehicle_observation(K, RANGE, frame=1, goals=np.float32([25.0, 0.0]))
        b.run(3)
        b.snapshot()
        scene_mask = torch.zeros(B, dtype=torch.bool, device="cuda")
        scene_mask[::8] = True
        if args.part == "paths":
            print(f"# {args.label}: vehicle episodes never set, {what} ({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            forms = (("run, per tick", lambda: b.run(args.ticks), 1, args.ticks), ("end_step()", b.end_step, calls, 1),
                     ("restart_device()", lambda: b.restart_device(scene_mask), calls, 1), ("observe_vehicles()", b.observe_vehicles, calls, 1))
            for name, fn, c, per in forms:
                fn()
                for r in range(args.rounds):
                    print(f"{args.label:<8} {name:<32} {r:>5} {_timed(fn, c) / per * 1e6:>10.2f}", flush=True)
            return
        veh_mask = torch.zeros(M, dtype=torch.bool, device="cuda")
        veh_mask[::8] = True
        every = np.ones(M, bool)
        one = np.zeros(M, bool)
        one[::M_B] = True
        wall = dict(RADII, wall_radius=0.3)
        goals = np.float32([25.0, 0.0])
        if args.part == "trace":
            b.set_vehicle_episodes(one, goals=goals, **wall)
            t1 = _timed(b.end_vehicle_step, calls)
            b.set_vehicle_episodes(every, goals=goals, **wall)
            t4 = _timed(b.end_vehicle_step, calls)
            u = _timed(lambda: b.respawn_vehicles_device(veh_mask), calls)
            print(f"# trace: {calls} end_vehicle_step() calls with one agent per scene: {t1 * 1e6:.1f} us per call; {calls} with every vehicle an "
                  f"agent: {t4 * 1e6:.1f} us per call; {calls} respawns of 1/8 of the vehicles: {u * 1e6:.1f} us per call (wall clock, under "
                  f"the tracer); {what}")
            return
        obs = b.vehicle_observation_tensor()
        age = torch.zeros(M, dtype=torch.int32, device="cuda")

        def torch_today():                                              # examples/batch_av_loop.py, behind its second observe_vehicles()
            nonlocal age
            goal_d2 = obs[:, 0] * obs[:, 0] + obs[:, 1] * obs[:, 1]
            hit = obs[:, 8] < 0.4 * 0.4
            near = (obs[:, 8] < 1.0) & ~hit
            arrived = goal_d2 < 2.0 * 2.0
            age += 1
            late = age >= 400
            done = hit | arrived | late
            age = torch.where(done, torch.zeros_like(age), age)
            return done, near

        names = ("one tick", "end_step()", "observe_vehicles()", "end_vehicle_step(), one agent vehicle per scene",
                 "end_vehicle_step(), all 4 096 vehicles agents", "respawn_vehicles_device(), 1/8 of the vehicles",
                 "torch today (batch_av_loop.py): goal, ring clearance, age, done")
        got = {n: [] for n in names}
        print(f"# vehicles: {what}; us per call")
        print(f"{'form':<72} {'round':>5} {'us/call':>12}")
        for r in range(args.rounds):
            got[names[0]].append(_timed(lambda: b.run(args.ticks), 1) / args.ticks)
            got[names[1]].append(_timed(b.end_step, calls))
            got[names[2]].append(_timed(b.observe_vehicles, calls))
            b.set_vehicle_episodes(one, goals=goals, **wall)
            b.end_vehicle_step()
            got[names[3]].append(_timed(b.end_vehicle_step, calls))
            b.set_vehicle_episodes(every, goals=goals, **wall)
            b.end_vehicle_step()
            got[names[4]].append(_timed(b.end_vehicle_step, calls))
            got[names[5]].append(_timed(lambda: b.respawn_vehicles_device(veh_mask), calls))
            torch_today()
            got[names[6]].append(_timed(torch_today, calls))
            b.restart_device(torch.ones(B, dtype=torch.bool, device="cuda"))
            for n in names:
                print(f"{n:<72} {r:>5} {got[n][-1] * 1e6:>12.1f}", flush=True)
        rec, done, sd = b.vehicle_episodes()
        print(f"# the latest end_vehicle_step: {int(done.sum())} of {M} vehicles done in {int(sd.sum())} of {B} scenes")
        print("# medians (us)")
        for n in names:
            print(f"{n:<72} {'med':>5} {statistics.median(got[n]) * 1e6:>12.1f}")
    finally:
        b.close()


if __name__ == "__main__":
    main()
