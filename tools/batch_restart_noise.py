"""Restart noise on a batch (sfm_batch_set_restart_noise): B = 1024 scenes of 64, all five forces, 4 moving device-side vehicles per
scene, every eighth scene chosen.
  --part run     `rounds` rounds of `calls` restart_device() calls with noise OFF, and of one run(ticks) call -- what a batch that
                 never sets restart noise launches; run once per library build (SFM_LIB_PATH names another build) and alternated by
                 tools/batch_restart_noise.sh: this build against its parent
  --part noise   alternated in `rounds` rounds (us per call, medians at the end): restart_device() with noise off; with noise on
                 (tries 8, gaps 0.6 m / 0.3 m, boxes of 1 m, goal boxes of 3 m); and the host path a caller had before: download,
                 the NumPy twin for the chosen scenes, upload, and setting steering, observation, episodes and scan again
  --part trace   `calls` restart_device() calls with noise on -- for rocprofv3 --kernel-trace --stats: the noise kernel's own duration
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
from carla_social_force_model_amd.batch import STEER_PREFERRED, SfmBatch  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402

POOL = 32
DT = 0.05
N_B = 64
K = 4
RANGE = 5.0
POS_BOX, GOAL_BOX, MIN_GAP, POINT_GAP, TRIES = (1.0, 1.0), (3.0, 3.0), 0.6, 0.3, 8


def _sync():
    import torch
    torch.cuda.synchronize()


def _timed(fn):
    _sync()
    t0 = time.perf_counter()
    fn()
    _sync()
    return time.perf_counter() - t0


def _scenes(B):
    pool = [vars(scenarios.make_scenario(N_B, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0))) for k in range(POOL)]
    return [pool[k % POOL] for k in range(B)]


def _sensors(b, kinds):
    b.set_steering(kinds)
    b.set_observation(K, RANGE)
    b.set_episodes(0, 1.0, 0.3, 0.3, 0)
    b.set_scan(10.0, 0.3, R=16, mask=[np.array([0])] * b.B)


def _noise_on(b):
    b.set_restart_noise(2024 + np.arange(b.B), np.array(POS_BOX), np.array(GOAL_BOX), MIN_GAP, POINT_GAP, TRIES)


def _host_reset(b, scenes, held, chosen, episode, kinds):
    """What a caller did before: everything to the host, the chosen scenes drawn there, everything up again."""
    from carla_social_force_model_amd import reset
    state, wps, veh = b.state(), b.waypoints(), b.dynamic_obstacles()
    new = []
    for k, sc in enumerate(scenes):
        sc = dict(sc)
        if chosen[k]:
            xy, wp, _, _, _ = reset.resample_scene(sc, 2024 + k, episode, np.array(POS_BOX), np.array(GOAL_BOX), MIN_GAP, POINT_GAP, TRIES,
                                                   state=held[0][k], vehicles=held[2][k], waypoints=held[1][k][0])
            loc = held[0][k][0].copy()
            loc[:, :2] = xy
            sc.update(loc=loc, vel=held[0][k][1], waypoint=np.column_stack([wp.astype(np.float64), np.zeros(len(wp))]),
                      dynamic_obstacles=held[2][k])
        else:
            sc.update(loc=state[k][0], vel=state[k][1], waypoint=np.column_stack([wps[k][0].astype(np.float64), np.zeros(len(wps[k][0]))]),
                      dynamic_obstacles=veh[k])
        new.append(sc)
    b.upload(new, device_vehicles=True)
    _sensors(b, kinds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("run", "noise", "trace"), default="noise")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    ap.add_argument("--scenes", type=int, default=1024)
    args = ap.parse_args()
    import torch
    B = args.scenes
    what = f"B = {B} scenes of {N_B}, all five forces, 4 moving device-side vehicles per scene, every eighth scene chosen"
    scenes = _scenes(B)
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        b.upload(scenes, device_vehicles=True)
        b.run(3)
        b.snapshot()
        mask = np.zeros(B, bool)
        mask[::8] = True
        d_mask = torch.from_numpy(mask).cuda()

        def restarts():
            for _ in range(args.calls):
                b.restart_device(d_mask)

        if args.part == "run":
            print(f"# {args.label}: noise off, {what} ({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            restarts()
            b.run(3)
            for r in range(args.rounds):
                t = _timed(restarts) / args.calls
                u = _timed(lambda: b.run(args.ticks)) / args.ticks
                print(f"{args.label:<8} {B:>6} {N_B:>5} {r:>5} {t * 1e6:>14.1f} {u * 1e6:>10.1f}", flush=True)
        elif args.part == "noise":
            print(f"# noise: {what}; tries {TRIES}, gaps {MIN_GAP} m / {POINT_GAP} m, boxes {POS_BOX[0]} m, goal boxes {GOAL_BOX[0]} m; us per call")
            print(f"{'form':<64} {'round':>5} {'us/call':>12}")
            kinds = np.zeros(B * N_B, np.uint8)
            kinds[::N_B] = STEER_PREFERRED
            _sensors(b, kinds)
            held = (b.state(), b.waypoints(), b.dynamic_obstacles())
            names = ("restart_device(), noise off", "restart_device(), noise on", "the host path: download, twin, upload, sensors again")
            got = {n: [] for n in names}
            restarts()
            for r in range(args.rounds):
                b.set_restart_noise(None, None)
                got[names[0]].append(_timed(restarts) / args.calls)
                _noise_on(b)
                restarts()
                got[names[1]].append(_timed(restarts) / args.calls)
                fallbacks = int(b.restart_noise()[1].sum())
                got[names[2]].append(_timed(lambda: _host_reset(b, scenes, held, mask, r, kinds)))
                b.snapshot()
                for n in names:
                    print(f"{n:<64} {r:>5} {got[n][-1] * 1e6:>12.1f}", flush=True)
            print(f"# rows of the latest noisy restarts that no try could place: {fallbacks} of {int(mask.sum()) * N_B}")
            print("# medians (us), and each over the first")
            ref = statistics.median(got[names[0]])
            for n in names:
                m = statistics.median(got[n])
                print(f"{n:<64} {'med':>5} {m * 1e6:>12.1f} {m / ref:>9.2f}x")
        else:
            _noise_on(b)
            t = _timed(restarts) / args.calls
            print(f"# trace: {args.calls} restart_device() calls with noise on, {what}: {t * 1e6:.1f} us per call (wall clock, under the tracer)")
    finally:
        b.close()


if __name__ == "__main__":
    main()
