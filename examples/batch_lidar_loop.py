"""The device loop of batch_rl_loop_device.py with a range scan as the policy's view of its surroundings.

    python examples/batch_lidar_loop.py [--scenes 256] [--steps 200] [--repeat 4] [--rays 16]

The same task -- B scenes of 64 pedestrians, row 0 of every scene the agent -- but the agent no longer reads a list of neighbours:
it reads R rays around itself, each the distance to the first pedestrian, kerb point, obstacle point or vehicle point it meets
(carla_social_force_model_amd.batch, "Range scans").  Only the agent rows are scanned (``mask``), so the scan costs what B rows
cost, not what the crowd costs.  Per step:
    observe(); scan()             two launches: the agents' goal and speed (k = 1 record), and their R ranges and kinds
    policy                        torch, on the same stream: towards the goal, pushed back along every ray that ends inside 1.5 m
    run(repeat)                   `repeat` ticks on the held command, one launch per tick
    end_step(auto_restart=True)   two launches: who is done and why, then the restart of exactly those scenes from the snapshot
Nothing crosses to the host inside the loop.
Needs an MI355X; importing this file does not."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from batch_rl_loop import GOAL_RADIUS, N_B, SENSE_RANGE, make_scenes  # noqa: E402  (the same task)
from batch_rl_loop_device import PED_RADIUS, VEH_RADIUS  # noqa: E402

RAYS = 16
KEEP_OFF = 1.5           # a ray that ends nearer than this pushes the agent back along itself, metres


def policy(goal, speed, ranges, dirs):
    """The agents' goal entries (B, 2), target speeds (B, 1), ranges (B, R) and the ray directions (R, 2), world axes -> preferred
    velocities (B, 2): towards the goal at the target speed, pushed back along every ray that ends inside KEEP_OFF."""
    to_goal = goal / goal.norm(dim=1, keepdim=True).clamp_min(1e-6)
    push = (KEEP_OFF - ranges).clamp_min(0.0) @ dirs * (-2.0 / dirs.shape[0])
    return speed * to_goal + push


def run(B=256, steps=200, repeat=4, max_age=150, rays=RAYS, device=0, quiet=False):
    import torch
    from carla_social_force_model_amd import scan as S, scenarios
    from carla_social_force_model_amd.batch import (EP_DONE, EP_REASON, REASON_ARRIVED, STEER_PREFERRED, SfmBatch)
    from carla_social_force_model_amd.config import default_sfm_config

    scenes = make_scenes(B)
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), 0.05, device=device, B=B)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)          # torch and the batch on one stream: launches and reads are ordered
        b.upload(scenes, device_vehicles=True)
        kinds = np.zeros(B * N_B, np.uint8)
        kinds[::N_B] = STEER_PREFERRED                                  # the agents; everyone else is not steered
        b.set_steering(kinds)
        b.set_observation(1, SENSE_RANGE)                               # the goal and the target speed come from this record
        b.set_scan(SENSE_RANGE, ped_radius=PED_RADIUS, R=rays, mask=kinds != 0)      # the agents' rows only, world axes
        b.set_episodes(agent=0, goal_radius=GOAL_RADIUS, ped_radius=PED_RADIUS, veh_radius=VEH_RADIUS, max_steps=max_age)
        b.snapshot()                                                    # the reset state of every scene
        obs, scan, cmd, rec = b.observation_tensor(), b.scan_tensor(), b.command_tensor(), b.episode_tensor()
        dirs = torch.as_tensor(np.stack(S.ray_directions(S.default_angles(rays)), axis=1), device=obs.device)
        agents = torch.arange(B, device=obs.device) * N_B
        tally = torch.zeros(2, dtype=torch.int64, device=obs.device)   # episodes ended, of them at the goal
        for step in range(steps):
            b.observe()
            b.scan()
            mine = obs[agents]
            cmd[agents, 0:2] = policy(mine[:, 0:2], mine[:, 4:5], scan[agents, :rays], dirs)
            b.run(repeat)
            b.end_step(auto_restart=True)                               # the record keeps the terminal values of the restarted scenes
            ended = rec[:, EP_DONE] != 0
            tally[0] += ended.sum()
            tally[1] += (ended & ((rec[:, EP_REASON].to(torch.int32) & REASON_ARRIVED) != 0)).sum()
        last, _ = b.episodes()                                          # the one copy of the record, after the loop
        episodes, arrivals = (int(v) for v in tally.cpu())
        if not quiet:
            print(f"{B} scenes of {N_B}, {steps} steps of {repeat} ticks, {rays} rays per agent: {episodes} episodes ended, "
                  f"{arrivals} of them at the goal; {int(last[:, EP_DONE].sum())} ended in the last step")
        return episodes, arrivals
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=4)
    ap.add_argument("--rays", type=int, default=RAYS)
    args = ap.parse_args()
    run(args.scenes, args.steps, args.repeat, rays=args.rays)


if __name__ == "__main__":
    main()
