"""Row episodes and row respawns on a batch (sfm_batch_end_row_step, sfm_batch_respawn_rows_device): B = 1024 scenes of 64, all five
forces, 4 moving device-side vehicles per scene.
  --part paths   `rounds` rounds of `calls` calls of what existed before, with row episodes never set: run(ticks) per tick, end_step(),
                 restart_device() of every eighth scene with noise off and with noise on -- run once per library build
                 (SFM_LIB_PATH names another build) and alternated by tools/batch_row_episodes.sh: this build against its parent
  --part rows    alternated in `rounds` rounds (us per call, medians at the end): end_step(), restart_device() and one tick beside
                 end_row_step() with one agent per scene and with every row an agent, respawn_rows_device() of 1/8 of the rows with
                 noise off and with noise on (tries 8, gaps 0.6 m / 0.3 m), the torch sequence a caller has today for the same
                 quantities (cdist over state_tensor() per scene, a row-wise minimum, a gather of snapshot rows), and one step of
                 examples/batch_multiagent_loop.py (observe, policy, 4 ticks, end_row_step(auto_respawn=True))
  --part trace   `calls` calls of end_row_step() (every row an agent) and of the noisy respawn -- for rocprofv3 --kernel-trace --stats
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
sys.path.insert(0, os.path.join(ROOT, "examples"))

from carla_social_force_model_amd import scenarios  # noqa: E402
from carla_social_force_model_amd.batch import STEER_PREFERRED, SfmBatch, obs_width  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402

POOL, DT, N_B, K, RANGE = 32, 0.05, 64, 4, 5.0
POS_BOX, MIN_GAP, POINT_GAP, TRIES = (1.0, 1.0), 0.6, 0.3, 8
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
    pool = [vars(scenarios.make_scenario(N_B, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0))) for k in range(POOL)]
    return [pool[k % POOL] for k in range(B)]


def _noise(b, on):
    if on:
        b.set_restart_noise(2024 + np.arange(b.B), np.array(POS_BOX), None, MIN_GAP, POINT_GAP, TRIES)
    else:
        b.set_restart_noise(None, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("paths", "rows", "trace"), default="rows")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    ap.add_argument("--scenes", type=int, default=1024)
    args = ap.parse_args()
    import torch
    B, calls = args.scenes, args.calls
    what = f"B = {B} scenes of {N_B}, all five forces, 4 moving device-side vehicles per scene"
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        b.upload(_scenes(B), device_vehicles=True)
        b.set_episodes(0, **RADII)
        b.run(3)
        b.snapshot()
        scene_mask = torch.zeros(B, dtype=torch.bool, device="cuda")
        scene_mask[::8] = True
        row_mask = torch.zeros(B * N_B, dtype=torch.bool, device="cuda")
        row_mask[::8] = True
        if args.part == "paths":
            print(f"# {args.label}: row episodes never set, {what} ({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            forms = (("run, per tick", lambda: b.run(args.ticks), 1, args.ticks, None), ("end_step()", b.end_step, calls, 1, None),
                     ("restart_device(), noise off", lambda: b.restart_device(scene_mask), calls, 1, False),
                     ("restart_device(), noise on", lambda: b.restart_device(scene_mask), calls, 1, True))
            for name, fn, c, per, noise in forms:
                if noise is not None:
                    _noise(b, noise)
                fn()
                for r in range(args.rounds):
                    print(f"{args.label:<8} {name:<32} {r:>5} {_timed(fn, c) / per * 1e6:>10.2f}", flush=True)
            return
        all_rows = np.ones(B * N_B, bool)
        one_row = np.zeros(B * N_B, bool)
        one_row[::N_B] = True
        if args.part == "trace":
            b.set_row_episodes(all_rows, **RADII)
            _noise(b, True)
            t = _timed(b.end_row_step, calls)
            u = _timed(lambda: b.respawn_rows_device(row_mask), calls)
            print(f"# trace: {calls} end_row_step() calls, every row an agent: {t * 1e6:.1f} us per call; {calls} noisy respawns of 1/8 of the rows: "
                  f"{u * 1e6:.1f} us per call (wall clock, under the tracer); {what}")
            return
        from batch_multiagent_loop import make_policy, rewards
        b.set_steering(np.full(B * N_B, STEER_PREFERRED, np.uint8))
        b.set_observation(K, RANGE)
        obs, cmd, state = b.observation_tensor(), b.command_tensor(), b.state_tensor()
        policy = make_policy(obs_width(K), obs.device)
        held = state.clone()                                            # the torch sequence's own copy of the snapshot rows
        idx = torch.nonzero(row_mask).squeeze(1)
        ret = torch.zeros(B * N_B, device="cuda")

        def torch_today():
            xy = state[:, :2].reshape(B, N_B, 2)
            d = torch.cdist(xy, xy)
            d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
            near = d.min(dim=2).values                                  # every row's nearest pedestrian
            state[idx] = held[idx]                                      # ... and 1/8 of the rows back to the snapshot
            return near

        def loop_step():
            nonlocal ret
            b.observe()
            cmd[:, 0:2] = policy(obs)
            b.run(4)
            b.end_row_step(auto_respawn=True)
            ret += rewards(rec)

        names = ("one tick", "end_step()", "restart_device(), every eighth scene, noise off", "end_row_step(), one agent per scene",
                 "end_row_step(), every row an agent", "respawn_rows_device(), 1/8 of the rows, noise off",
                 "respawn_rows_device(), 1/8 of the rows, noise on", "torch today: cdist per scene, row-wise min, gather of snapshot rows",
                 "one step of examples/batch_multiagent_loop.py")
        got = {n: [] for n in names}
        print(f"# rows: {what}; tries {TRIES}, gaps {MIN_GAP} m / {POINT_GAP} m, boxes {POS_BOX[0]} m; us per call")
        print(f"{'form':<72} {'round':>5} {'us/call':>12}")
        for r in range(args.rounds):
            _noise(b, False)
            got[names[0]].append(_timed(lambda: b.run(args.ticks), 1) / args.ticks)
            got[names[1]].append(_timed(b.end_step, calls))
            got[names[2]].append(_timed(lambda: b.restart_device(scene_mask), calls))
            b.set_row_episodes(one_row, **RADII)
            b.end_row_step()
            got[names[3]].append(_timed(b.end_row_step, calls))
            b.set_row_episodes(all_rows, **RADII)
            rec = b.row_episode_tensor()
            b.end_row_step()
            got[names[4]].append(_timed(b.end_row_step, calls))
            got[names[5]].append(_timed(lambda: b.respawn_rows_device(row_mask), calls))
            _noise(b, True)
            b.respawn_rows_device(row_mask)
            got[names[6]].append(_timed(lambda: b.respawn_rows_device(row_mask), calls))
            fallbacks = int(b.row_respawns()[1].sum())
            torch_today()
            got[names[7]].append(_timed(torch_today, calls))
            loop_step()
            got[names[8]].append(_timed(loop_step, calls))
            b.restart_device(torch.ones(B, dtype=torch.bool, device="cuda"))
            for n in names:
                print(f"{n:<72} {r:>5} {got[n][-1] * 1e6:>12.1f}", flush=True)
        print(f"# rows of the latest noisy respawn that no try could place: {fallbacks} of {int(row_mask.sum())}")
        print("# medians (us)")
        for n in names:
            print(f"{n:<72} {'med':>5} {statistics.median(got[n]) * 1e6:>12.1f}")
    finally:
        b.close()


if __name__ == "__main__":
    main()
