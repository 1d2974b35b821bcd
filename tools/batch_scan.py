"""Range scans on a batch (sfm_batch_set_scan, sfm_batch_scan, SFM_BATCH_PTR_SCAN): B = 1024 scenes of 64, R = 32 rays, a range limit
of 5 m, pedestrians as discs of 0.3 m and geometry points as discs of 0.1 m, all five forces, 4 moving device-side vehicles per scene.
  --part run     `rounds` rounds of one run(ticks) call of the batch WITHOUT scans -- run once per library build (SFM_LIB_PATH
                 names another build) and alternated by tools/batch_scan.sh: this build against its parent
  --part scan    alternated in `rounds` rounds of `ticks` scans each (us per scan, medians at the end):
                 (a) scan() of one agent row per scene (mask), pedestrians and all three geometry kinds;
                 (r) scan() of every row, the same;
                 (o) observe() of the same batch (k = 8), for scale;
                 (ta) what a caller had before, in torch on the same stream from state_tensor(), for the agent rows: the (B, 1, 64, R)
                      ray-disc intermediates over the pedestrians, a masked minimum.  Pedestrian discs only: the polylines and the
                      device-side vehicle rings are not reachable from torch;
                 (tr) the same for every row, through the (B, 64, 64, R) intermediates
  --part trace   3 warm-up ticks, then `ticks` x (run(1), observe(), scan() of the agents, scan() of every row) -- for rocprofv3
                 --kernel-trace: the duration of one sfm_batch_scan_kernel launch of each form beside one observe and one tick
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


def _torch_scan(state, B, dirs, rows):
    """The ranges as a caller built them before, pedestrian discs only: (B, rows, R), RANGE where a ray meets nobody nearer."""
    import torch
    s = state.view(B, N_B, 4)
    p = s[:, :, :2]
    a = p[:, None, :, :] - p[:, :rows, None, :]                        # (B, rows, 64, 2)
    t = a[..., 0:1] * dirs[:, 0] + a[..., 1:2] * dirs[:, 1]             # (B, rows, 64, R): the intermediates
    c = a[..., 0:1] * dirs[:, 1] - a[..., 1:2] * dirs[:, 0]
    q = PED_RADIUS * PED_RADIUS - c * c
    w = q.clamp_min(0.0).sqrt()
    me = torch.eye(N_B, dtype=torch.bool, device=s.device)[:rows]
    cand = (q > 0) & (t + w > 0) & ~me[None, :, :, None]
    rng = torch.where(cand, (t - w).clamp_min(0.0), torch.full((), float("inf"), device=s.device))
    return rng.amin(dim=2).clamp_max(RANGE)


def _medians(got, base):
    print("# medians (us), and each over the first")
    ref = statistics.median(got[base])
    for name, ts in got.items():
        m = statistics.median(ts)
        print(f"{name:<52} {'med':>5} {m * 1e6:>12.1f} {m / ref:>9.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("run", "scan", "trace"), default="scan")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    B = 1024
    what = f"B = {B} scenes of {N_B}, all five forces, 4 moving device-side vehicles per scene"
    batches = []
    try:
        if args.part == "run":
            print(f"# {args.label}: run({args.ticks}) without scans, {what} "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            b = _batch(B)
            batches.append(b)
            b.run(3)
            for r in range(args.rounds):
                t = _timed(lambda: b.run(args.ticks)) / args.ticks
                print(f"{args.label:<8} {B:>6} {N_B:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
        elif args.part == "scan":
            import torch
            from carla_social_force_model_amd import scan as S
            print(f"# scans: {what}; R = {R} rays, range limit {RANGE} m, pedestrian discs {PED_RADIUS} m, point discs {POINT_RADIUS} m; "
                  f"{args.ticks} scans per round, us per scan")
            print(f"{'form':<52} {'round':>5} {'us/scan':>12}")
            one, every = _batch(B), _batch(B)
            batches += [one, every]
            for b, mask in ((one, _agents(B)), (every, None)):
                b.set_stream(torch.cuda.current_stream().cuda_stream)
                b.set_scan(RANGE, PED_RADIUS, POINT_RADIUS, R=R, mask=mask)
                b.set_observation(K, RANGE)
                b.run(3)
            state = every.state_tensor()
            dirs = torch.as_tensor(np.stack(S.ray_directions(S.default_angles(R)), axis=1), device=state.device)

            def repeat(fn):
                def go():
                    for _ in range(args.ticks):
                        fn()
                return go

            forms = (("a: scan(), one agent row per scene", repeat(one.scan)),
                     ("r: scan(), every row", repeat(every.scan)),
                     ("o: observe(), k = 8, every row", repeat(every.observe)),
                     ("ta: torch, pedestrian discs only, agent rows", repeat(lambda: _torch_scan(state, B, dirs, 1))),
                     ("tr: torch, pedestrian discs only, every row", repeat(lambda: _torch_scan(state, B, dirs, N_B))))
            got = {n: [] for n, _ in forms}
            for _, fn in forms:                                        # warm-up: torch's allocator and kernels, the first launches
                fn()
            for r in range(args.rounds):
                for name, fn in forms:
                    t = _timed(fn) / args.ticks
                    got[name].append(t)
                    print(f"{name:<52} {r:>5} {t * 1e6:>12.1f}", flush=True)
            _medians(got, "a: scan(), one agent row per scene")
            # the torch form and the kernel agree where only pedestrians are in the way (torch rounds in another order: a few ulp)
            ours = every.scan_tensor().view(B, N_B, 2 * R)
            theirs = _torch_scan(state, B, dirs, N_B)
            ped_only = ours[:, :, R:] <= 1
            close = ((ours[:, :, :R] - theirs).abs() <= 1e-3) | ~ped_only
            print(f"# rays that end on a pedestrian or on nothing: {100 * ped_only.float().mean().item():.1f} %; of them within 1 mm of the "
                  f"torch form: {100 * (close & ped_only).float().sum().item() / ped_only.float().sum().item():.2f} %")
        else:
            b, c = _batch(B), _batch(B)
            batches += [b, c]
            b.set_scan(RANGE, PED_RADIUS, POINT_RADIUS, R=R, mask=_agents(B))
            c.set_scan(RANGE, PED_RADIUS, POINT_RADIUS, R=R)
            b.set_observation(K, RANGE)
            b.run(3)
            c.run(3)
            _sync()
            n = args.ticks

            def steps():
                for _ in range(n):
                    b.run(1)
                    b.observe()
                    b.scan()
                    c.scan()

            t = _timed(steps)
            print(f"# trace: {what}: {n} x (run(1), observe(), scan() of one agent row per scene, scan() of every row of a second batch "
                  f"in the same state after 3 ticks); {t * 1e6 / n:.1f} us per step (wall clock, under the tracer).  In the kernel trace "
                  f"the scan launches alternate: agents, every row")
    finally:
        for b in batches:
            b.close()


if __name__ == "__main__":
    main()
