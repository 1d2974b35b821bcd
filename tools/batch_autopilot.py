"""The vehicle autopilot on a batch (sfm_batch_set_vehicle_autopilot): B = 1024 scenes of 64, all five forces, 4 moving device-side
vehicles per scene.
  --part run     `rounds` rounds of one run(ticks) call of the batch with the autopilot NEVER set -- run once per library build
                 (SFM_LIB_PATH names another build) and alternated by tools/batch_autopilot.sh: this build against its parent
  --part pilot   alternated in `rounds` rounds of one run(ticks) each, three batches of the same scenes (us per tick, medians at the
                 end): (0) no vehicle autopiloted, the autopilot never set; (1) ONE vehicle per scene autopiloted; (4) all four
  --part old     the path a caller had before, per tick, on the same batch, alternated with (4): observe_vehicles(), a torch IDM on
                 the nearest pedestrian only, the commands written through vehicle_command_tensor(), run(1) -- everything on the
                 device, one stream, `ticks` ticks per round
  --part trace   3 warm-up ticks, then run(ticks) with every vehicle autopiloted -- for rocprofv3 --kernel-trace: one
                 sfm_batch_vehicle_autopilot_kernel launch in front of every tick
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

POOL = 32
DT = 0.05
N_B = 64
M_B = 4
SET = dict(v0=6.0, T=1.0, s0=2.0, acc=1.5, dec=2.0, brake=6.0, half_width=1.5, front=2.5, look=30.0, reach=3.0, ped_margin=0.5,
           max_turn=0.05)


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
    pool = [vars(scenarios.make_scenario(N_B, 7000 + k, n_borders=2, n_static=2, n_dynamic=M_B, border_len=(2.0, 2.0))) for k in range(POOL)]
    return [pool[k % POOL] for k in range(B)]


def _paths(scenes, piloted):
    """A closed square of 30 m about each scene's crowd for the first ``piloted`` vehicles of every scene, None for the others."""
    out = []
    for sc in scenes:
        mid = sc["loc"][:, :2].mean(axis=0)
        square = mid + 15.0 * np.array([[1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0], [1.0, -1.0]])
        out.append([np.roll(square, -k, axis=0) if k < piloted else None for k in range(M_B)])
    return out


def _batch(B, piloted=0):
    scenes = _scenes(B)
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    b.upload(scenes, device_vehicles=True)
    if piloted:
        b.set_vehicle_autopilot(_paths(scenes, piloted), loop=True, **SET)
    return b


def _medians(got, base):
    print("# medians (us), and each over the first")
    ref = statistics.median(got[base])
    for name, ts in got.items():
        m = statistics.median(ts)
        print(f"{name:<60} {'med':>5} {m * 1e6:>12.1f} {m / ref:>9.2f}x")


def _alternate(forms, rounds, per):
    got = {n: [] for n, _ in forms}
    for _, fn in forms:                                                # warm-up: the first launches
        fn()
    for r in range(rounds):
        for name, fn in forms:
            t = _timed(fn) / per
            got[name].append(t)
            print(f"{name:<60} {r:>5} {t * 1e6:>12.1f}", flush=True)
    _medians(got, forms[0][0])


def _torch_policy(b, ticks):
    """The caller's own controller: per tick observe_vehicles(), an IDM in torch against the NEAREST pedestrian only (slot 0 of the
    record, in the heading frame), the commands written into vehicle_command_tensor(), run(1)."""
    import torch
    b.set_stream(torch.cuda.current_stream().cuda_stream)
    b.set_vehicle_driving(2, np.float32([0.0, 1.0, 0.0]))
    b.set_vehicle_observation(1, SET["look"], frame=1)
    cmd, obs = b.vehicle_command_tensor(), b.vehicle_observation_tensor()
    v0, T, s0, acc, dec, brake = (SET[k] for k in ("v0", "T", "s0", "acc", "dec", "brake"))
    k2 = 2.0 * (acc * dec) ** 0.5

    def go():
        for _ in range(ticks):
            b.observe_vehicles()
            s = obs[:, 15].clamp_min(0.0)                              # the signed speed along the heading
            al, ac, u = obs[:, 16], obs[:, 17], obs[:, 18] + obs[:, 15]
            led = (obs[:, 7] > 0) & (al > 0) & (ac.abs() < SET["half_width"] + SET["ped_margin"])
            gap = ((al - SET["front"]) - SET["ped_margin"]).clamp_min(0.01)
            sstar = s0 + (s * T + s * (s - u) / k2).clamp_min(0.0)
            inter = torch.where(led, (sstar / gap) ** 2, torch.zeros_like(s))
            a = (acc * (1.0 - (s / v0) ** 4 - inter)).clamp_min(-brake)
            cmd[:, 0] = (s + DT * a).clamp_min(0.0)
            b.run(1)
    return go


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("run", "pilot", "old", "trace"), default="pilot")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    ap.add_argument("--scenes", type=int, default=1024)
    args = ap.parse_args()
    ticks, B = args.ticks, args.scenes
    what = f"B = {B} scenes of {N_B}, all five forces, {M_B} moving device-side vehicles per scene"
    batches = []
    try:
        if args.part == "run":
            print(f"# {args.label}: run({ticks}), the autopilot never set, {what} "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            b = _batch(B)
            batches.append(b)
            b.run(3)
            for r in range(args.rounds):
                t = _timed(lambda: b.run(ticks)) / ticks
                print(f"{args.label:<8} {B:>6} {N_B:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
        elif args.part == "pilot":
            print(f"# autopilot: {what}; run({ticks}) per round, us per tick")
            print(f"{'form':<60} {'round':>5} {'us/tick':>12}")
            forms = []
            for name, piloted in (("0: no vehicle autopiloted (never set)", 0), ("1: one vehicle per scene autopiloted", 1),
                                  ("4: every vehicle autopiloted", 4)):
                b = _batch(B, piloted)
                batches.append(b)
                b.run(3)
                forms.append((name, (lambda b=b: b.run(ticks))))
            _alternate(forms, args.rounds, ticks)
        elif args.part == "old":
            print(f"# the caller's own controller against the autopilot: {what}; {ticks} ticks per round, us per tick")
            print(f"{'form':<60} {'round':>5} {'us/tick':>12}")
            a, b = _batch(B, 4), _batch(B)
            batches += [a, b]
            a.run(3)
            _alternate((("4: every vehicle autopiloted, run(ticks)", lambda: a.run(ticks)),
                        ("t: observe_vehicles() + torch IDM (nearest only) + run(1)", _torch_policy(b, ticks))), args.rounds, ticks)
        else:
            b = _batch(B, 4)
            batches.append(b)
            b.run(3)
            t = _timed(lambda: b.run(ticks))
            print(f"# trace: {what}, every vehicle autopiloted: 3 warm-up ticks, then run({ticks}); "
                  f"{t * 1e6 / ticks:.1f} us per tick (wall clock, under the tracer)")
    finally:
        for b in batches:
            b.close()


if __name__ == "__main__":
    main()
