"""Bird's-eye grids around the vehicles of a batch (sfm_batch_set_vehicle_grid, sfm_batch_grid_vehicles): B = 1024 scenes of 64, all
five forces, 4 moving device-side vehicles per scene.
  --part run     `rounds` rounds of one run(ticks) call, of `ticks` grid() calls (one agent row per scene, 32 x 32) and of `ticks`
                 scan_vehicles() calls (one ego vehicle per scene, 64 rays) -- run once per library build (SFM_LIB_PATH names
                 another build) and alternated process by process: this build against its parent
  --part grid    alternated in `rounds` rounds of `ticks` calls each (us per call, medians at the end): grid_vehicles() with one ego
                 vehicle per scene at 32 x 32 and at 48 x 20 with a forward centre, and with every vehicle at 32 x 32 (three batches
                 of the same scenes), and on the first batch grid() of one agent row per scene (32 x 32) and scan_vehicles() of one
                 ego vehicle per scene (64 rays)
  --part torch   alternated likewise: grid_vehicles() with one ego vehicle per scene, 32 x 32, world axes, and the torch sequence a
                 caller had before -- the pedestrian channels only, from state_tensor() and the vehicle centres, through (B, M, N)
                 intermediates and index_add_
  --part trace   3 warm-up calls each, then `ticks` grid_vehicles() calls of each of the three forms of --part grid, in that
                 order -- for a kernel trace in a run of its own
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
CELL = 0.5
RMAX = 10.0
PED_R = 0.3
FORWARD = (8.0, 0.0)
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
            print(f"{name:<72} {r:>5} {t * 1e6:>12.1f}", flush=True)
    print("# medians (us), and each over the first")
    ref = statistics.median(got[forms[0][0]])
    for name, ts in got.items():
        m = statistics.median(ts)
        print(f"{name:<72} {'med':>5} {m * 1e6:>12.1f} {m / ref:>9.2f}x")


def _grid_forms(B, batches):
    """The three vehicle-grid batches of --part grid and --part trace: [(name, batch)]."""
    forms = []
    for name, GU, GV, centre, mask in (("e32: grid_vehicles(), one ego per scene, 32 x 32", 32, 32, (0.0, 0.0), EGO * B),
                                       ("e48: grid_vehicles(), one ego per scene, 48 x 20, centre (8, 0)", 48, 20, FORWARD, EGO * B),
                                       ("a32: grid_vehicles(), every vehicle (4 096), 32 x 32", 32, 32, (0.0, 0.0), None)):
        b = _batch(B)
        batches.append(b)
        b.set_vehicle_grid(CELL, GU, GV, mask=mask, frame=1, centre=centre)
        b.run(3)
        forms.append((name, b))
    return forms


def _torch_grid(state, centres, vel, G, cell):
    """The pedestrian channels only, world axes, around the vehicle centres: (B, M, 3, G, G) through (B, M, N) intermediates and
    index_add_ (float atomics: the sums depend on the order the hardware takes)."""
    import torch
    B, N = state.shape[0], state.shape[1]
    M = centres.shape[1]
    a = state[:, None, :, 0:2] - centres[:, :, None, :]
    p = a / cell + 0.5 * G
    inside = ((p >= 0) & (p < G)).all(dim=-1)
    cid = (p[..., 1].long().clamp(0, G - 1) * G + p[..., 0].long().clamp(0, G - 1))
    rv = state[:, None, :, 2:4] - vel[:, :, None, :]
    slot = torch.arange(B * M, device=state.device).view(B, M, 1) * (G * G)
    flat = (slot + cid)[inside]
    out = torch.zeros(3, B * M * G * G, device=state.device)
    out[0].index_add_(0, flat, torch.ones_like(flat, dtype=torch.float32))
    out[1].index_add_(0, flat, rv[..., 0][inside])
    out[2].index_add_(0, flat, rv[..., 1][inside])
    return out.view(3, B, M, G, G).permute(1, 2, 0, 3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("run", "grid", "torch", "trace"), default="grid")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    ticks, B = args.ticks, 1024
    what = f"B = {B} scenes of {N_B}, all five forces, {M_B} moving device-side vehicles per scene"
    batches = []
    try:
        if args.part == "run":
            print(f"# {args.label}: run({ticks}), {ticks} x grid() (one agent row per scene, 32 x 32) and {ticks} x scan_vehicles() "
                  f"(one ego per scene, 64 rays), {what} "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            b = _batch(B)
            batches.append(b)
            b.set_grid(CELL, G=32, mask=[[0]] * B, frame=1)
            b.set_vehicle_scan(RMAX, PED_R, R=64, mask=EGO * B, frame=1, mount=(2.0, 0.0))
            b.run(3)
            b.grid()
            b.scan_vehicles()
            for r in range(args.rounds):
                t = _timed(lambda: b.run(ticks)) / ticks
                g = _timed(_repeat(b.grid, ticks)) / ticks
                s = _timed(_repeat(b.scan_vehicles, ticks)) / ticks
                print(f"{args.label:<8} {B:>6} {N_B:>5} {r:>5} {t * 1e6:>10.1f} {g * 1e6:>10.1f} {s * 1e6:>10.1f}", flush=True)
        elif args.part == "grid":
            print(f"# sensors: {what}; {CELL} m cells, heading frame; {ticks} calls per round, us per call")
            print(f"{'form':<72} {'round':>5} {'us/call':>12}")
            forms = _grid_forms(B, batches)
            first = forms[0][1]
            first.set_grid(CELL, G=32, mask=[[0]] * B, frame=1)
            first.set_vehicle_scan(RMAX, PED_R, R=64, mask=EGO * B, frame=1, mount=(2.0, 0.0))
            calls = [(name, _repeat(b.grid_vehicles, ticks)) for name, b in forms]
            calls += [("g: grid(), one agent row per scene, 32 x 32", _repeat(first.grid, ticks)),
                      ("s: scan_vehicles(), one ego per scene, 64 rays", _repeat(first.scan_vehicles, ticks))]
            _alternate(calls, args.rounds, ticks)
        elif args.part == "torch":
            import torch
            print(f"# pedestrian channels only: {what}; one ego per scene, 32 x 32, world axes; {ticks} calls per round, us per call")
            print(f"{'form':<72} {'round':>5} {'us/call':>12}")
            b = _batch(B)
            batches.append(b)
            b.set_stream(torch.cuda.current_stream().cuda_stream)
            b.set_vehicle_grid(CELL, 32, 32, mask=EGO * B)
            b.run(3)
            state = b.state_tensor().view(B, N_B, 4)
            centres = torch.as_tensor(np.array([[veh[0][0]] for veh in b.dynamic_obstacles()], dtype=np.float32), device=state.device)
            vel = torch.as_tensor(np.array([d[3][0:1] for d in _velocities(b)], dtype=np.float32), device=state.device)
            ours = b.vehicle_grid_tensor()
            b.grid_vehicles()
            theirs = _torch_grid(state, centres, vel, 32, CELL)
            _sync()
            moved = int((ours[:, 0] != theirs[:, 0, 0]).sum())
            gap = float((ours[:, 1:3] - theirs[:, 0, 1:3]).abs().max())
            print(f"# counts differ in {moved} cells of {ours[:, 0].numel()}, the sums agree to {gap:.2e} m/s "
                  f"(the torch sequence contracts, and its adds come in the order the hardware takes)")
            _alternate((("k: grid_vehicles(), one launch", _repeat(b.grid_vehicles, ticks)),
                        ("t: the torch sequence over state_tensor()", _repeat(lambda: _torch_grid(state, centres, vel, 32, CELL), ticks))),
                       args.rounds, ticks)
        else:
            forms = _grid_forms(B, batches)
            for _, b in forms:
                for _ in range(3):
                    b.grid_vehicles()
            _sync()
            for name, b in forms:
                t = _timed(_repeat(b.grid_vehicles, ticks))
                print(f"# trace: {name}: {ticks} calls, {t * 1e6 / ticks:.1f} us per call (wall clock, under the tracer)")
    finally:
        for b in batches:
            b.close()


def _velocities(b):
    """Per scene (kind, command, heading, velocity) of the vehicles: driving is switched on with every vehicle left alone, which is
    what vehicle_driving() needs."""
    b.set_vehicle_driving(0)
    return b.vehicle_driving()


if __name__ == "__main__":
    main()
