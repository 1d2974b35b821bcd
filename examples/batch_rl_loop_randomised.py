"""The loop of batch_rl_loop_device.py with resets that sample: every episode of a scene starts from another draw.

    python examples/batch_rl_loop_randomised.py [--scenes 256] [--steps 200] [--repeat 4]

The same task, policy and loop as examples/batch_rl_loop_device.py -- observe, act, step, end_step(auto_restart=True), nothing on the
host -- with restart noise set (carla_social_force_model_amd.batch, "Restart noise"): the auto restart is followed by one more launch
that draws every pedestrian's start from a box of +-1 m around its snapshot position, again while it would stand nearer than 0.6 m to
somebody or 0.3 m to a kerb, obstacle or vehicle point, and every goal from a box of +-3 m around the snapshot goal.  Without it the
crowd of a scene replays the identical motion in every episode until the agent's own actions perturb it; with it a scene is a
distribution of episodes, keyed by (seed, restart counter) and therefore reproducible.  The counters stay on the device too.
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
from batch_rl_loop_device import PED_RADIUS, VEH_RADIUS  # noqa: E402

POS_BOX = (1.0, 1.0)     # half-extents of the box a start is drawn from, metres
GOAL_BOX = (3.0, 3.0)    # ... and a goal
MIN_GAP = 0.6            # no two starts nearer than this, metres
POINT_GAP = 0.3          # no start nearer than this to a border, obstacle or vehicle point
TRIES = 8


def run(B=256, steps=200, repeat=4, max_age=150, device=0, seed=2024, quiet=False):
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
        b.set_restart_noise(seed + np.arange(B), np.array(POS_BOX), np.array(GOAL_BOX), MIN_GAP, POINT_GAP, TRIES)
        b.snapshot()                                                    # the state the starts are drawn around
        b.restart()                                                     # the first episodes are draws as well
        obs, cmd, rec = b.observation_tensor(), b.command_tensor(), b.episode_tensor()
        agents = torch.arange(B, device=obs.device) * N_B
        tally = torch.zeros(2, dtype=torch.int64, device=obs.device)   # episodes ended, of them at the goal
        for step in range(steps):
            b.observe()
            cmd[agents, 0:2] = policy(obs[agents])
            b.run(repeat)
            b.end_step(auto_restart=True)                               # the restart, then the draw, of exactly the scenes that are done
            ended = rec[:, EP_DONE] != 0
            tally[0] += ended.sum()
            tally[1] += (ended & ((rec[:, EP_REASON].to(torch.int32) & REASON_ARRIVED) != 0)).sum()
        resets, fallbacks = b.restart_noise()                           # the one copy of the counters, after the loop
        episodes, arrivals = (int(v) for v in tally.cpu())
        if not quiet:
            print(f"{B} scenes of {N_B}, {steps} steps of {repeat} ticks: {episodes} episodes ended, {arrivals} of them at the goal; "
                  f"{int(resets.sum())} restarts drawn, {int(fallbacks.sum())} rows of the latest ones at their snapshot position")
        return episodes, arrivals, resets, fallbacks
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
