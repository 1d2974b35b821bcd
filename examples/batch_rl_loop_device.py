"""The RL-style loop of batch_rl_loop.py with nothing left on the host: observe, act, step, decide who is done, reset.

    python examples/batch_rl_loop_device.py [--scenes 256] [--steps 200] [--repeat 4]

The same task as examples/batch_rl_loop.py -- B scenes of 64 pedestrians, row 0 of every scene the agent, the same hand-written
policy -- with the episode ends decided by the library (carla_social_force_model_amd.batch, "Episode ends"):
    observe()                     one launch: every row's record
    policy                        torch, on the same stream, observation_tensor() -> command_tensor()
    run(repeat)                   `repeat` ticks on the held command, one launch per tick
    end_step(auto_restart=True)   two launches: who is done (goal reached, out of time, touched a pedestrian or a vehicle, no
                                  longer live) and why, then the restart of exactly those scenes from the snapshot
Nothing crosses to the host inside the loop: no `.cpu()`, no age tensor, no mask.  The tally is kept in a torch tensor on the
device, and one (B, 8) episode record and that tally are copied at the end.
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

from batch_rl_loop import GOAL_RADIUS, K, N_B, SENSE_RANGE, make_scenes, policy  # noqa: E402  (the same task, the same policy)

PED_RADIUS = 0.3         # the agent touches a pedestrian closer than this (centre to centre), metres
VEH_RADIUS = 0.3         # ... or a vehicle ring point closer than this


def run(B=256, steps=200, repeat=4, max_age=150, device=0, quiet=False):
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
        b.set_observation(K, SENSE_RANGE)
        b.set_episodes(agent=0, goal_radius=GOAL_RADIUS, ped_radius=PED_RADIUS, veh_radius=VEH_RADIUS, max_steps=max_age)
        b.snapshot()                                                    # the reset state of every scene
        obs, cmd, rec = b.observation_tensor(), b.command_tensor(), b.episode_tensor()
        agents = torch.arange(B, device=obs.device) * N_B
        tally = torch.zeros(2, dtype=torch.int64, device=obs.device)   # episodes ended, of them at the goal
        for step in range(steps):
            b.observe()
            cmd[agents, 0:2] = policy(obs[agents])
            b.run(repeat)
            b.end_step(auto_restart=True)                               # the record keeps the terminal values of the restarted scenes
            ended = rec[:, EP_DONE] != 0
            tally[0] += ended.sum()
            tally[1] += (ended & ((rec[:, EP_REASON].to(torch.int32) & REASON_ARRIVED) != 0)).sum()
        last, _ = b.episodes()                                          # the one copy of the record, after the loop
        episodes, arrivals = (int(v) for v in tally.cpu())
        if not quiet:
            print(f"{B} scenes of {N_B}, {steps} steps of {repeat} ticks: {episodes} episodes ended, {arrivals} of them at the goal; "
                  f"{int(last[:, EP_DONE].sum())} ended in the last step")
        return episodes, arrivals
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=4)
    args = ap.parse_args()
    run(args.scenes, args.steps, args.repeat)


if __name__ == "__main__":
    main()
