"""Occupancy grids on a batch (sfm_batch_set_grid, sfm_batch_grid, SFM_BATCH_PTR_GRID): B = 1024 scenes of 64, G = 16 cells of 0.5 m,
the row's heading frame, all five forces, 4 moving device-side vehicles per scene.
  --part existing  `rounds` rounds of run(ticks), `ticks` x scan(), `ticks` x observe() and `ticks` x restart_device() of a batch WITHOUT
                   grids -- run once per library build (SFM_LIB_PATH names another build) and alternated by tools/batch_grid.sh: this
                   build against its parent
  --part grid      alternated in `rounds` rounds of `ticks` calls each (us per call, medians at the end):
                   (a) grid() of one agent row per scene (mask): pedestrians, their velocities and all three geometry kinds;
                   (r) grid() of every row, the same;
                   (o) observe() (k = 8), (s) scan() (R = 32, every row) and (t) one tick of the same batch, for scale;
                   (ta) what a caller had before, in torch on the same stream from state_tensor(), for the agent rows: subtract,
                        rotate, bucketise, index_add_ through (B, 1, 64) intermediates.  Pedestrian channels only: the polylines
                        and the device-side vehicle rings are not reachable from torch; float atomics, so not reproducible;
                   (tr) the same for every row, through (B, 64, 64) intermediates
  --part trace     3 warm-up ticks, then `ticks` x (run(1), observe(), scan(), grid() of the agents, grid() of every row of a second
                   batch) -- for rocprofv3 --kernel-trace: the duration of one sfm_batch_grid_kernel launch of each form beside one
                   observe, one scan and one tick
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
G = 16
CELL = 0.5
FRAME = 1
R = 32
RANGE = 5.0
PED_RADIUS = 0.3
POINT_RADIUS = 0.1
K = 8


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


def _batch(B):
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    b.upload(_scenes(B), device_vehicles=True)
    return b


def _agents(B):
    mask = np.zeros(B * N_B, bool)
    mask[::N_B] = True
    return mask


def _torch_grid(state, B, rows):
    """The pedestrian channels as a caller built them before: (B, rows, 3, G, G) -- count and the summed relative velocity per cell,
    in the heading frame (v / |v|, the world's axes for a row at rest: the goal is not in the state)."""
    import torch
    s = state.view(B, N_B, 4)
    p, v = s[:, :, :2], s[:, :, 2:]
    me = s[:, :rows]
    speed = me[:, :, 2:].norm(dim=2, keepdim=True)
    h = torch.where(speed > 0, me[:, :, 2:] / speed.clamp_min(1e-30), torch.tensor([1.0, 0.0], device=s.device))     # (B, rows, 2)
    hx, hy = h[:, :, None, 0], h[:, :, None, 1]
    a = p[:, None, :, :] - me[:, :, None, :2]                          # (B, rows, 64, 2): the intermediates
    w = v[:, None, :, :] - me[:, :, None, 2:]
    fx, fy = hx * a[..., 0] + hy * a[..., 1], hx * a[..., 1] - hy * a[..., 0]
    wx, wy = hx * w[..., 0] + hy * w[..., 1], hx * w[..., 1] - hy * w[..., 0]
    pu, pv = fx / CELL + 0.5 * G, fy / CELL + 0.5 * G
    inside = (pu >= 0) & (pu < G) & (pv >= 0) & (pv < G) & ~torch.eye(N_B, dtype=torch.bool, device=s.device)[:rows]
    cell = pv.clamp(0, G - 1).long() * G + pu.clamp(0, G - 1).long()
    slot = torch.arange(B * rows, device=s.device).view(B, rows, 1) * (3 * G * G)
    out = torch.zeros(B * rows * 3 * G * G, device=s.device)
    one = inside.float()
    for ch, val in enumerate((one, wx * one, wy * one)):
        out.index_add_(0, (slot + ch * G * G + cell).reshape(-1), val.reshape(-1))
    return out.view(B, rows, 3, G, G)


def _medians(got, base):
    print("# medians (us), and each over the first")
    ref = statistics.median(got[base])
    for name, ts in got.items():
        m = statistics.median(ts)
        print(f"{name:<56} {'med':>5} {m * 1e6:>12.1f} {m / ref:>9.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("existing", "grid", "trace"), default="grid")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    B = 1024
    what = f"B = {B} scenes of {N_B}, all five forces, 4 moving device-side vehicles per scene"
    batches = []

    def repeat(fn):
        def go():
            for _ in range(args.ticks):
                fn()
        return go

    try:
        if args.part == "existing":
            import torch
            print(f"# {args.label}: the paths that existed, without grids, {what} "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'}); us per call")
            b = _batch(B)
            batches.append(b)
            b.set_stream(torch.cuda.current_stream().cuda_stream)
            b.set_scan(RANGE, PED_RADIUS, POINT_RADIUS, R=R)
            b.set_observation(K, RANGE)
            b.run(3)
            b.snapshot()
            every = torch.ones(B, dtype=torch.uint8, device="cuda")
            forms = ((f"run({args.ticks}), per tick", lambda: b.run(args.ticks)), ("scan(), every row", repeat(b.scan)),
                     ("observe(), k = 8", repeat(b.observe)), ("restart_device(), every scene", repeat(lambda: b.restart_device(every))))
            for _, fn in forms:
                fn()
            for r in range(args.rounds):
                for name, fn in forms:
                    t = _timed(fn) / args.ticks
                    print(f"{args.label:<8} {name:<32} {r:>5} {t * 1e6:>10.1f}", flush=True)
        elif args.part == "grid":
            import torch
            print(f"# grids: {what}; G = {G} cells of {CELL} m, frame {FRAME}; {args.ticks} calls per round, us per call")
            print(f"{'form':<56} {'round':>5} {'us/call':>12}")
            one, every = _batch(B), _batch(B)
            batches += [one, every]
            for b, mask in ((one, _agents(B)), (every, None)):
                b.set_stream(torch.cuda.current_stream().cuda_stream)
                b.set_grid(CELL, G=G, mask=mask, frame=FRAME)
                b.set_scan(RANGE, PED_RADIUS, POINT_RADIUS, R=R)
                b.set_observation(K, RANGE)
                b.run(3)
            state = every.state_tensor()
            forms = (("a: grid(), one agent row per scene", repeat(one.grid)),
                     ("r: grid(), every row", repeat(every.grid)),
                     ("o: observe(), k = 8, every row", repeat(every.observe)),
                     ("s: scan(), R = 32, every row", repeat(every.scan)),
                     ("ta: torch, pedestrian channels only, agent rows", repeat(lambda: _torch_grid(state, B, 1))),
                     ("tr: torch, pedestrian channels only, every row", repeat(lambda: _torch_grid(state, B, N_B))),
                     ("t: one tick (last: it moves the state)", lambda: every.run(args.ticks)))
            got = {n: [] for n, _ in forms}
            for _, fn in forms[:-1]:                                   # warm-up: torch's allocator and kernels, the first launches
                fn()
            for r in range(args.rounds):
                for name, fn in forms:
                    t = _timed(fn) / args.ticks
                    got[name].append(t)
                    print(f"{name:<56} {r:>5} {t * 1e6:>12.1f}", flush=True)
            _medians(got, "a: grid(), one agent row per scene")
            # the torch form and the kernel agree on the pedestrian counts of the rows that walk (torch's heading has no goal)
            every.grid()
            ours = every.grid_tensor().view(B, N_B, 6, G, G)[:, :, 0]
            theirs = _torch_grid(every.state_tensor(), B, N_B)[:, :, 0]
            same = (ours == theirs).flatten(2).all(dim=2)
            print(f"# rows whose pedestrian counts equal the torch form's in every cell: {100 * same.float().mean().item():.2f} % "
                  f"(the torch form rounds its rotation in another order; {int(ours.sum().item())} sources binned in all)")
            print(f"# buffer: {one.grid_tensor().numel() * 4 / 2 ** 20:.1f} MiB for the agents, "
                  f"{every.grid_tensor().numel() * 4 / 2 ** 20:.1f} MiB for every row")
        else:
            b, c = _batch(B), _batch(B)
            batches += [b, c]
            b.set_grid(CELL, G=G, mask=_agents(B), frame=FRAME)
            c.set_grid(CELL, G=G, frame=FRAME)
            b.set_observation(K, RANGE)
            b.set_scan(RANGE, PED_RADIUS, POINT_RADIUS, R=R)
            b.run(3)
            c.run(3)
            _sync()
            n = args.ticks

            def steps():
                for _ in range(n):
                    b.run(1)
                    b.observe()
                    b.scan()
                    b.grid()
                    c.grid()

            t = _timed(steps)
            print(f"# trace: {what}: {n} x (run(1), observe(), scan() of every row, grid() of one agent row per scene, grid() of every "
                  f"row of a second batch in the same state after 3 ticks); {t * 1e6 / n:.1f} us per step (wall clock, under the "
                  f"tracer).  In the kernel trace the grid launches alternate: agents, every row")
    finally:
        for b in batches:
            b.close()


if __name__ == "__main__":
    main()
