"""The device loop of batch_lidar_loop.py with an occupancy grid as the policy's view of its surroundings.

    python examples/batch_grid_loop.py [--scenes 256] [--steps 200] [--repeat 4] [--cells 16]

The same task -- B scenes of 64 pedestrians, row 0 of every scene the agent -- but the agent reads a local map: a G x G grid of
0.5 m cells centred on itself, 6 channels (carla_social_force_model_amd.batch, "Occupancy grids").  Only the agent rows are gridded
(``mask``), so the buffer is (B, 6, G, G) -- one slot per agent, the layout a convolution takes as it stands.  Per step:
    observe(); grid()             two launches: the agents' goal and speed (k = 1 record), and their local maps
    policy                        torch, on the same stream: a small conv layer over the map, read out as a push away from what is near
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

CELLS = 16
CELL = 0.5               # metres
KEEP_OFF = 1.5           # what is nearer than this pushes the agent away, metres


def conv_policy_weights(G, cell, device):
    """The policy's two layers.  A 3 x 3 convolution, 6 channels in and 2 out: channel 0 smooths "somebody is here" (pedestrian
    count, weight 1), channel 1 "something is here" (border, obstacle and vehicle points, 0.25 each: they are sampled 0.1 m apart);
    the velocity channels are not used.  And a readout (2 G^2, 2): every cell pushes the agent away from itself, by
    (KEEP_OFF - distance)+ / distance along the direction to the cell's centre.  Returns (kernel (2, 54), readout (2 G^2, 2))."""
    import torch
    k = torch.zeros(2, 6, 3, 3)
    k[0, 0] = 1.0 / 9.0
    k[1, 3:6] = 0.25 / 9.0
    centre = (np.arange(G) + 0.5 - G / 2.0) * cell
    ux, vy = np.meshgrid(centre, centre)                               # cell [cv][cu]: u along x, v along y
    d = np.maximum(np.hypot(ux, vy), 0.5 * cell)
    w = np.clip(KEEP_OFF - d, 0.0, None) / d ** 2
    away = -np.stack([w * ux, w * vy], axis=-1).reshape(G * G, 2)
    return k.reshape(2, 54).to(device), torch.as_tensor(np.concatenate([away, away]), dtype=torch.float32, device=device)


def policy(goal, speed, maps, kernel, readout):
    """The agents' goal entries (B, 2), target speeds (B, 1) and maps (B, 6, G, G), world axes -> preferred velocities (B, 2):
    towards the goal at the target speed, pushed away from what the conv layer finds near.  The convolution is written as an
    im2col and a matrix product, so it needs no tuned convolution library."""
    import torch
    import torch.nn.functional as F
    B, _, G, _ = maps.shape
    to_goal = goal / goal.norm(dim=1, keepdim=True).clamp_min(1e-6)
    cols = F.unfold(maps, kernel_size=3, padding=1)                    # (B, 54, G^2)
    feat = torch.relu(kernel @ cols).reshape(B, 2 * G * G)             # (B, 2, G^2): the conv layer and its ReLU
    return speed * to_goal + feat @ readout


def run(B=256, steps=200, repeat=4, max_age=150, cells=CELLS, device=0, quiet=False):
    import torch
    from carla_social_force_model_amd import scenarios
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
        b.set_grid(CELL, G=cells, mask=kinds != 0)                      # the agents' rows only, world axes: slot s is scene s's agent
        b.set_episodes(agent=0, goal_radius=GOAL_RADIUS, ped_radius=PED_RADIUS, veh_radius=VEH_RADIUS, max_steps=max_age)
        b.snapshot()                                                    # the reset state of every scene
        obs, maps, cmd, rec = b.observation_tensor(), b.grid_tensor(), b.command_tensor(), b.episode_tensor()
        assert maps.shape == (B, 6, cells, cells) and np.array_equal(b.grid_rows(), np.arange(B) * N_B)
        kernel, readout = conv_policy_weights(cells, CELL, obs.device)
        agents = torch.arange(B, device=obs.device) * N_B
        tally = torch.zeros(2, dtype=torch.int64, device=obs.device)   # episodes ended, of them at the goal
        for step in range(steps):
            b.observe()
            b.grid()
            mine = obs[agents]
            cmd[agents, 0:2] = policy(mine[:, 0:2], mine[:, 4:5], maps, kernel, readout)
            b.run(repeat)
            b.end_step(auto_restart=True)                               # the record keeps the terminal values of the restarted scenes
            ended = rec[:, EP_DONE] != 0
            tally[0] += ended.sum()
            tally[1] += (ended & ((rec[:, EP_REASON].to(torch.int32) & REASON_ARRIVED) != 0)).sum()
        last, _ = b.episodes()                                          # the one copy of the record, after the loop
        episodes, arrivals = (int(v) for v in tally.cpu())
        if not quiet:
            print(f"{B} scenes of {N_B}, {steps} steps of {repeat} ticks, a {cells} x {cells} map per agent: {episodes} episodes ended, "
                  f"{arrivals} of them at the goal; {int(last[:, EP_DONE].sum())} ended in the last step")
        return episodes, arrivals
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=4)
    ap.add_argument("--cells", type=int, default=CELLS)
    args = ap.parse_args()
    run(args.scenes, args.steps, args.repeat, cells=args.cells)


if __name__ == "__main__":
    main()
