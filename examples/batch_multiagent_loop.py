"""Decentralised multi-agent crowd navigation with nothing left on the host: EVERY pedestrian of every scene is an agent.

    python examples/batch_multiagent_loop.py [--scenes 256] [--steps 200] [--repeat 4]

The crowd of examples/batch_rl_loop.py -- B scenes of 64 pedestrians with vehicles -- where every row is steered (kind 2: the command
is the row's preferred velocity) by ONE small policy network shared by all agents (CADRL-style parameter sharing), and every row has
its own goal, collision test and time limit (carla_social_force_model_amd.batch, "Row episodes"):
    observe()                         one launch: every row's record
    policy                            torch, on the same stream, observation_tensor() -> command_tensor(), all B * 64 rows at once
    run(repeat)                       `repeat` ticks on the held commands, one launch per tick
    end_row_step(auto_respawn=True)   two launches: which AGENTS are done and why, then exactly those rows back from the snapshot
                                      (with restart noise: placed again around their starts, clear of the crowd as it stands now)
                                      while their scenes go on
The reward of every agent is formed on the device from its row of the record: progress towards the goal, a bonus for arriving, a
penalty for touching a pedestrian or a vehicle.  Nothing crosses to the host inside the loop; the return and the tally are copied
once, with one `.cpu()`, after it.
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

from batch_rl_loop import GOAL_RADIUS, K, N_B, SENSE_RANGE, make_scenes  # noqa: E402  (the same crowd)

PED_RADIUS = 0.3         # an agent touches a pedestrian closer than this (centre to centre), metres
VEH_RADIUS = 0.3         # ... or a vehicle ring point closer than this
MAX_SPEED = 1.4          # the policy's commands are preferred velocities of at most this, m/s
HIDDEN = 32


def make_policy(width, device, seed=0):
    """The shared policy: observation row -> preferred velocity, a two-layer network with fixed random weights (a stand-in for a
    trained one: the loop around it is the point)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    w1 = (torch.randn(width, HIDDEN, generator=g) / width ** 0.5).to(device)
    w2 = (torch.randn(HIDDEN, 2, generator=g) / HIDDEN ** 0.5).to(device)

    def policy(obs):
        x = torch.nan_to_num(obs, nan=0.0, posinf=0.0, neginf=0.0).clamp_(-SENSE_RANGE, SENSE_RANGE)
        return MAX_SPEED * torch.tanh(torch.tanh(x @ w1) @ w2)
    return policy


def rewards(rec):
    """Per-agent reward from the row record (N_total, 8), on the device."""
    import torch
    from carla_social_force_model_amd.batch import (EP_GOAL_D2, EP_PREV_GOAL_D2, EP_REASON, REASON_ARRIVED, REASON_PED_HIT, REASON_VEH_HIT)
    reason = rec[:, EP_REASON].to(torch.int32)
    progress = torch.nan_to_num(rec[:, EP_PREV_GOAL_D2].sqrt() - rec[:, EP_GOAL_D2].sqrt(), nan=0.0, posinf=0.0, neginf=0.0)
    return (progress + 10.0 * ((reason & REASON_ARRIVED) != 0) - 5.0 * ((reason & (REASON_PED_HIT | REASON_VEH_HIT)) != 0))


def run(B=256, steps=200, repeat=4, max_age=150, device=0, noise=True, quiet=False):
    import torch
    from carla_social_force_model_amd import scenarios
    from carla_social_force_model_amd.batch import EP_DONE, STEER_PREFERRED, SfmBatch, obs_width
    from carla_social_force_model_amd.config import default_sfm_config

    scenes = make_scenes(B)
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), 0.05, device=device, B=B)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)          # torch and the batch on one stream: launches and reads are ordered
        b.upload(scenes, device_vehicles=True)
        b.set_steering(np.full(B * N_B, STEER_PREFERRED, np.uint8))    # every row is steered
        b.set_observation(K, SENSE_RANGE)
        b.set_row_episodes(True, goal_radius=GOAL_RADIUS, ped_radius=PED_RADIUS, veh_radius=VEH_RADIUS, max_steps=max_age)
        if noise:                                                       # a respawned agent starts near its start, clear of the others
            b.set_restart_noise(np.arange(B, dtype=np.uint32) + 1, (0.6, 0.6), min_gap=0.6, point_gap=0.3, tries=8)
        b.snapshot()                                                    # the reset state of every row
        obs, cmd, rec = b.observation_tensor(), b.command_tensor(), b.row_episode_tensor()
        policy = make_policy(obs_width(K), obs.device)
        ret = torch.zeros(B * N_B, device=obs.device)                  # every agent's return
        tally = torch.zeros(1, device=obs.device)                      # agent episodes ended
        for step in range(steps):
            b.observe()
            cmd[:, 0:2] = policy(obs)
            b.run(repeat)
            b.end_row_step(auto_respawn=True)                           # the record keeps the terminal values of the respawned rows
            ret += rewards(rec)
            tally += (rec[:, EP_DONE] != 0).sum()
        out = torch.cat([tally, ret.mean().reshape(1)]).cpu()           # the one copy, after the loop
        episodes, mean_return = int(out[0]), float(out[1])
        if not quiet:
            print(f"{B} scenes of {N_B} agents, {steps} steps of {repeat} ticks: {episodes} agent episodes ended, mean return {mean_return:.3f}")
        return episodes, mean_return
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
