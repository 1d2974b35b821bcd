"""Driven vehicles and vehicle observations on a batch (sfm_batch_set_vehicle_driving, sfm_batch_observe_vehicles): B = 1024 scenes
of 64, all five forces, 4 moving device-side vehicles per scene.
  --part run     `rounds` rounds of one run(ticks) call of the batch WITHOUT driving -- run once per library build
                 (SFM_LIB_PATH names another build) and alternated by tools/batch_driving.sh: this build against its parent
  --part drive   alternated in `rounds` rounds of one run(ticks) each, three batches of the same scenes (us per tick, medians at the
                 end): (f) free running, driving off; (1) driving on, ONE vehicle per scene driven (kind 2), the others kind 0;
                 (a) every vehicle driven (kinds 1 and 2 alternating)
  --part obs     alternated in `rounds` rounds of `ticks` calls each (us per call): observe_vehicles() (K = 8, 5 m, every vehicle)
                 and observe() (K = 8, 5 m, every row) on the same batch
  --part old     the path a caller had before, per tick, on `ticks` ticks (default 2: the host part is slow): drive_vehicles on
                 the host for every scene, sfm_batch_set_dynamic_obstacles with the new rings, run(1), a download of the state,
                 and a NumPy nearest-pedestrian query per vehicle -- each timed on its own (us per tick)
  --part trace   3 warm-up ticks, then `ticks` x (run(1), observe(), observe_vehicles()) with every vehicle driven -- for
                 rocprofv3 --kernel-trace: one sfm_batch_vehicle_observe_kernel launch beside the tick and the row sensor
Times are host wall clock around the calls, closed by a device synchronisation."""
from __future__ import annotations

import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from carla_social_force_model_amd import scenarios  # noqa: E402
from carla_social_force_model_amd._lib import f32, fptr, iptr  # noqa: E402
from carla_social_force_model_amd.batch import SfmBatch  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402

POOL = 32
DT = 0.05
N_B = 64
M_B = 4
K = 8
RANGE = 5.0
TURN = (float(np.cos(0.02)), float(np.sin(0.02)))


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


def _batch(B, drive="none", device_vehicles=True):
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    b.upload(_scenes(B), device_vehicles=device_vehicles)
    if drive == "one":
        b.set_vehicle_driving([[2, 0, 0, 0]] * B, np.float32([3.0, *TURN]))
    elif drive == "all":
        b.set_vehicle_driving([[2, 1, 2, 1]] * B, [np.float32([[3.0, *TURN], [2.0, 1.0, 0.0], [-1.0, *TURN], [0.0, 0.0, 0.0]])] * B)
    return b


def _medians(got, base):
    print("# medians (us), and each over the first")
    ref = statistics.median(got[base])
    for name, ts in got.items():
        m = statistics.median(ts)
        print(f"{name:<52} {'med':>5} {m * 1e6:>12.1f} {m / ref:>9.2f}x")


def _alternate(forms, rounds, per):
    got = {n: [] for n, _ in forms}
    for _, fn in forms:                                                # warm-up: the first launches
        fn()
    for r in range(rounds):
        for name, fn in forms:
            t = _timed(fn) / per
            got[name].append(t)
            print(f"{name:<52} {r:>5} {t * 1e6:>12.1f}", flush=True)
    _medians(got, forms[0][0])


def _old_path(B, ticks):
    scenes = [copy.deepcopy(sc) for sc in _scenes(B)]
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    b.upload(scenes)                                                   # rings that stay: the host moves them
    kinds, cmds = [2, 1, 2, 1], np.float32([[3.0, *TURN], [2.0, 1.0, 0.0], [-1.0, *TURN], [0.0, 0.0, 0.0]])
    item_off = np.arange(B + 1, dtype=np.int32) * M_B
    parts = dict(host=[], upload=[], tick=[], download=[], query=[])
    try:
        b.run(1)
        for _ in range(ticks):
            t0 = time.perf_counter()
            for sc in scenes:
                scenarios.drive_vehicles(sc, kinds, cmds, DT)
            t1 = time.perf_counter()
            rings = [r for sc in scenes for _, r in sc["dynamic_obstacles"]]
            off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
            pts = np.concatenate(rings)
            ctr = np.array([c for sc in scenes for c, _ in sc["dynamic_obstacles"]])
            vel = np.concatenate([sc["dynamic_vel"] for sc in scenes])
            cols = [f32(pts[:, 0]), f32(pts[:, 1]), f32(ctr[:, 0]), f32(ctr[:, 1]), f32(vel[:, 0]), f32(vel[:, 1])]
            b._check(b._lib.sfm_batch_set_dynamic_obstacles(b._b, iptr(item_off), iptr(off), *(fptr(a) for a in cols)),
                     "sfm_batch_set_dynamic_obstacles")
            _sync()
            t2 = time.perf_counter()
            b.run(1)
            _sync()
            t3 = time.perf_counter()
            state = b.state()
            t4 = time.perf_counter()
            near = [np.argmin(((loc[None, :, :2] - np.array([c for c, _ in sc["dynamic_obstacles"]])[:, None, :]) ** 2).sum(axis=2), axis=1)
                    for (loc, _), sc in zip(state, scenes)]
            t5 = time.perf_counter()
            assert len(near) == B
            for name, t in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                parts[name].append(t)
    finally:
        b.close()
    print(f"{'step of the old path':<52} {'med':>5} {'us/tick':>12}")
    total = 0.0
    for name, label in (("host", "drive_vehicles on the host, every scene"), ("upload", "pack + sfm_batch_set_dynamic_obstacles"),
                        ("tick", "run(1)"), ("download", "state()"), ("query", "NumPy nearest pedestrian per vehicle")):
        m = statistics.median(parts[name])
        total += m
        print(f"{label:<52} {'med':>5} {m * 1e6:>12.1f}")
    print(f"{'sum':<52} {'med':>5} {total * 1e6:>12.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("run", "drive", "obs", "old", "trace"), default="drive")
    ap.add_argument("--ticks", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    ticks = args.ticks if args.ticks is not None else (2 if args.part == "old" else 50)
    B = 1024
    what = f"B = {B} scenes of {N_B}, all five forces, {M_B} moving device-side vehicles per scene"
    batches = []
    try:
        if args.part == "run":
            print(f"# {args.label}: run({ticks}) without driving, {what} "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            b = _batch(B)
            batches.append(b)
            b.run(3)
            for r in range(args.rounds):
                t = _timed(lambda: b.run(ticks)) / ticks
                print(f"{args.label:<8} {B:>6} {N_B:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
        elif args.part == "drive":
            print(f"# driving: {what}; run({ticks}) per round, us per tick")
            print(f"{'form':<52} {'round':>5} {'us/tick':>12}")
            forms = []
            for name, drive in (("f: free running, driving off", "none"), ("1: one vehicle per scene driven (kind 2)", "one"),
                                ("a: every vehicle driven (kinds 1 and 2)", "all")):
                b = _batch(B, drive)
                batches.append(b)
                b.run(3)
                forms.append((name, (lambda b=b: b.run(ticks))))
            _alternate(forms, args.rounds, ticks)
        elif args.part == "obs":
            print(f"# sensors: {what}; K = {K}, sense range {RANGE} m; {ticks} calls per round, us per call")
            print(f"{'form':<52} {'round':>5} {'us/call':>12}")
            b = _batch(B, "all")
            batches.append(b)
            b.set_observation(K, RANGE)
            b.set_vehicle_observation(K, RANGE, 1)
            b.run(3)

            def repeat(fn):
                def go():
                    for _ in range(ticks):
                        fn()
                return go

            _alternate((("v: observe_vehicles(), 4 096 vehicles", repeat(b.observe_vehicles)),
                        ("o: observe(), 65 536 rows", repeat(b.observe))), args.rounds, ticks)
        elif args.part == "old":
            print(f"# the old path: {what}, the vehicles moved by the host every tick; {ticks} ticks, medians, us per tick")
            _old_path(B, ticks)
        else:
            b = _batch(B, "all")
            batches.append(b)
            b.set_observation(K, RANGE)
            b.set_vehicle_observation(K, RANGE, 1)
            b.run(3)
            _sync()

            def steps():
                for _ in range(ticks):
                    b.run(1)
                    b.observe()
                    b.observe_vehicles()

            t = _timed(steps)
            print(f"# trace: {what}, every vehicle driven: 3 warm-up ticks, then {ticks} x (run(1), observe(), observe_vehicles()); "
                  f"{t * 1e6 / ticks:.1f} us per step (wall clock, under the tracer)")
    finally:
        for b in batches:
            b.close()


if __name__ == "__main__":
    main()
