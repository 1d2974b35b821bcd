"""An RL-style loop on a batch with no host copy of the state: observe, act, step, reset.

    python examples/batch_rl_loop.py [--scenes 256] [--steps 200] [--repeat 4]

B scenes of 64 pedestrians run in lock-step on one GPU.  Row 0 of every scene is the agent: a hand-written policy (walk to the goal
at the target speed, lean away from the nearest neighbour and from the nearest vehicle point) reads the observation tensor the
library fills on the device and writes the command tensor the ticks read; everyone else is an ordinary social-force pedestrian.
Per step:
    observe()                 one launch: every row's record (carla_social_force_model_amd.batch, "Observations")
    policy                    torch, on the same stream, observation_tensor() -> command_tensor()
    run(repeat)               `repeat` ticks on the held command (action repeat), one launch per tick
    restart(done)             the scenes whose agent reached its goal (or ran out of time) start over from the snapshot
The only thing that crosses to the host is the `done` mask (B bytes per step), because it chooses what to restart.
Needs an MI355X; importing this file does not."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_B = 64
K = 4
SENSE_RANGE = 5.0
GOAL_RADIUS = 1.0


def make_scenes(B, seed=0):
    from carla_social_force_model_amd import scenarios
    pool = [vars(scenarios.make_scenario(N_B, seed + k, n_borders=2, n_static=2, n_dynamic=2, border_len=(3.0, 8.0))) for k in range(min(B, 32))]
    return [pool[k % len(pool)] for k in range(B)]


def policy(obs):
    """Observation rows of the agents (B, 16 + 4K) -> preferred velocities (B, 2): towards the goal at the target speed, pushed back
    from the nearest neighbour (slot 0) and from the nearest vehicle point while they are inside 1.5 m."""
    import torch
    goal, speed = obs[:, 0:2], obs[:, 4:5]
    to_goal = goal / goal.norm(dim=1, keepdim=True).clamp_min(1e-6)

    def away(rel, there):
        d = rel.norm(dim=1, keepdim=True)
        return torch.where(there & (d < 1.5), -rel / d.clamp_min(1e-6) * (1.5 - d), torch.zeros_like(rel))

    push = away(obs[:, 16:18], obs[:, 6:7] > 0) + away(obs[:, 8:10], (obs[:, 7:8].to(torch.int32) & 4) != 0)
    return speed * to_goal + push


def run(B=256, steps=200, repeat=4, max_age=150, device=0, quiet=False):
    import torch
    from carla_social_force_model_amd import scenarios
    from carla_social_force_model_amd.batch import STEER_PREFERRED, SfmBatch
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
        b.snapshot()                                                    # the reset state of every scene
        obs, cmd = b.observation_tensor(), b.command_tensor()
        agents = torch.arange(B, device=obs.device) * N_B
        age = torch.zeros(B, dtype=torch.int32, device=obs.device)
        episodes = arrivals = 0
        for step in range(steps):
            b.observe()
            mine = obs[agents]
            arrived = mine[:, 0:2].norm(dim=1) < GOAL_RADIUS
            done = arrived | (age >= max_age) | (mine[:, 5] == 0)       # reached the goal, out of time, or no longer live
            cmd[agents, 0:2] = policy(mine)
            b.run(repeat)
            age += 1
            mask = done.cpu().numpy()                                   # the one copy to the host: who starts over
            if mask.any():
                b.restart(mask)
                age[done] = 0
                episodes += int(mask.sum())
                arrivals += int(arrived.sum().item())
        torch.cuda.synchronize()
        if not quiet:
            print(f"{B} scenes of {N_B}, {steps} steps of {repeat} ticks: {episodes} episodes ended, {arrivals} of them at the goal")
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
