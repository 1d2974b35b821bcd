"""Range scans from the vehicles of a batch (sfm_batch_set_vehicle_scan, sfm_batch_scan_vehicles): B = 1024 scenes of 64, all five
forces, 4 moving device-side vehicles per scene.
  --part run     `rounds` rounds of one run(ticks) call and of `ticks` scan() calls (one agent row per scene, 64 rays) -- run once
                 per library build (SFM_LIB_PATH names another build) and alternated by tools/batch_vehicle_scan.sh: this build
                 against its parent
  --part scan    alternated in `rounds` rounds of `ticks` calls each (us per call, medians at the end): scan_vehicles() with one ego
                 vehicle per scene at 64 and at 256 rays and with every vehicle at 64 rays (three batches of the same scenes), and
                 on the first batch scan() of one agent row per scene (64 rays) and observe_vehicles() (K = 8, every vehicle)
  --part torch   alternated likewise: scan_vehicles() with one ego vehicle per scene, 64 rays, pedestrian discs only, and the torch
                 sequence a caller had before -- the same discs from state_tensor() and the vehicle centres, through (B, M, N, R)
                 intermediates
  --part trace   3 warm-up calls each, then `ticks` scan_vehicles() calls of each of the three forms of --part scan, in that
                 order -- for rocprofv3 --kernel-trace
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
K = 8
RMAX = 10.0
PED_R = 0.3
MOUNT = (2.0, 0.0)
EGO = [[1, 0, 0, 0]]


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


def _batch(B):
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    b.upload(_scenes(B), device_vehicles=True)
    return b


def _repeat(fn, times):
    def go():
        for _ in range(times):
            fn()
    return go


def _alternate(forms, rounds, per):
    got = {n: [] for n, _ in forms}
    for _, fn in forms:                                                # warm-up: the first launches
        fn()
    for r in range(rounds):
        for name, fn in forms:
            t = _timed(fn) / per
            got[name].append(t)
            print(f"{name:<64} {r:>5} {t * 1e6:>12.1f}", flush=True)
    print("# medians (us), and each over the first")
    ref = statistics.median(got[forms[0][0]])
    for name, ts in got.items():
        m = statistics.median(ts)
        print(f"{name:<64} {'med':>5} {m * 1e6:>12.1f} {m / ref:>9.2f}x")


def _scan_forms(B, batches):
    """The three vehicle-scan batches of --part scan and --part trace: [(name, batch)]."""
    forms = []
    for name, R, mask in (("e64: scan_vehicles(), one ego per scene, 64 rays", 64, EGO * B),
                          ("e256: scan_vehicles(), one ego per scene, 256 rays", 256, EGO * B),
                          ("a64: scan_vehicles(), every vehicle (4 096), 64 rays", 64, None)):
        b = _batch(B)
        batches.append(b)
        b.set_vehicle_scan(RMAX, PED_R, R=R, mask=mask, frame=1, mount=MOUNT)
        b.run(3)
        forms.append((name, b))
    return forms


def _torch_scan(state, centres, dirs, r2, rmax):
    """Pedestrian discs only, world axes, from the vehicle centres: (B, M, R) ranges through (B, M, N, R) intermediates."""
    import torch
    p = state[:, :, 0:2]
    a = p[:, None, :, :] - centres[:, :, None, :]
    ax, ay = a[..., 0:1], a[..., 1:2]
    t = ax * dirs[:, 0] + ay * dirs[:, 1]
    c = ax * dirs[:, 1] - ay * dirs[:, 0]
    q = r2 - c * c
    w = torch.sqrt(q.clamp(min=0.0))
    cand = (q > 0) & (t + w > 0)
    rng = torch.where(cand, (t - w).clamp(min=0.0), torch.full_like(t, rmax))
    return rng.amin(dim=2).clamp(max=rmax)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("run", "scan", "torch", "trace"), default="scan")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    ticks, B = args.ticks, 1024
    what = f"B = {B} scenes of {N_B}, all five forces, {M_B} moving device-side vehicles per scene"
    batches = []
    try:
        if args.part == "run":
            print(f"# {args.label}: run({ticks}) and {ticks} x scan() (one agent row per scene, 64 rays), {what} "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            b = _batch(B)
            batches.append(b)
            b.set_scan(RMAX, PED_R, R=64, mask=[[0]] * B, frame=1)
            b.run(3)
            b.scan()
            for r in range(args.rounds):
                t = _timed(lambda: b.run(ticks)) / ticks
                s = _timed(_repeat(b.scan, ticks)) / ticks
                print(f"{args.label:<8} {B:>6} {N_B:>5} {r:>5} {t * 1e6:>10.1f} {s * 1e6:>10.1f}", flush=True)
        elif args.part == "scan":
            print(f"# sensors: {what}; range {RMAX} m, heading frame, mount {MOUNT}; {ticks} calls per round, us per call")
            print(f"{'form':<64} {'round':>5} {'us/call':>12}")
            forms = _scan_forms(B, batches)
            first = forms[0][1]
            first.set_scan(RMAX, PED_R, R=64, mask=[[0]] * B, frame=1)
            first.set_vehicle_observation(K, 5.0, 1)
            calls = [(name, _repeat(b.scan_vehicles, ticks)) for name, b in forms]
            calls += [("s: scan(), one agent row per scene, 64 rays", _repeat(first.scan, ticks)),
                      ("v: observe_vehicles(), 4 096 vehicles, K = 8", _repeat(first.observe_vehicles, ticks))]
            _alternate(calls, args.rounds, ticks)
        elif args.part == "torch":
            import torch
            from carla_social_force_model_amd import scan
            print(f"# pedestrian discs only: {what}; one ego per scene, 64 rays, world axes, no mount; {ticks} calls per round, us per call")
            print(f"{'form':<64} {'round':>5} {'us/call':>12}")
            b = _batch(B)
            batches.append(b)
            b.set_stream(torch.cuda.current_stream().cuda_stream)
            b.set_vehicle_scan(RMAX, PED_R, 0.0, R=64, mask=EGO * B)
            b.run(3)
            state = b.state_tensor().view(B, N_B, 4)
            centres = torch.as_tensor(np.array([[veh[0][0]] for veh in b.dynamic_obstacles()], dtype=np.float32), device=state.device)
            dirs = torch.as_tensor(np.stack(scan.ray_directions(scan.default_angles(64)), axis=1), device=state.device)
            r2 = float(scan.radius2(PED_R))
            ours = b.vehicle_scan_tensor()
            b.scan_vehicles()
            theirs = _torch_scan(state, centres, dirs, r2, RMAX)
            _sync()
            gap = float((ours.view(B, M_B, 128)[:, 0:1, :64] - theirs).abs().max())
            print(f"# the two agree to {gap:.2e} m (the torch sequence contracts and reorders freely)")
            _alternate((("k: scan_vehicles(), one launch", _repeat(b.scan_vehicles, ticks)),
                        ("t: the torch sequence over state_tensor()", _repeat(lambda: _torch_scan(state, centres, dirs, r2, RMAX), ticks))),
                       args.rounds, ticks)
        else:
            forms = _scan_forms(B, batches)
            for _, b in forms:
                for _ in range(3):
                    b.scan_vehicles()
            _sync()
            for name, b in forms:
                t = _timed(_repeat(b.scan_vehicles, ticks))
                print(f"# trace: {name}: {ticks} calls, {t * 1e6 / ticks:.1f} us per call (wall clock, under the tracer)")
    finally:
        for b in batches:
            b.close()


if __name__ == "__main__":
    main()
