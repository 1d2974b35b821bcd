"""The device loop of batch_rl_loop_device.py on a street with traffic that yields: autopiloted cars circulate on a closed path.

    python examples/batch_traffic_loop.py [--scenes 256] [--steps 200] [--repeat 4]

The same task as examples/batch_rl_loop_device.py -- B scenes of 64 pedestrians, row 0 of every scene the agent, the same
hand-written policy, the episode ends decided by the library -- but the scenes' vehicles are no longer boxes that drive through
whoever stands in their lane.  ``set_vehicle_autopilot`` gives each of them a closed path round the crowd; from then on every
integrating tick is preceded by one controller launch in which each car steps its cursor, turns towards its next waypoint and sets
its speed by the Intelligent Driver Model against the nearest pedestrian, vehicle ring or nothing in its corridor
(carla_social_force_model_amd.batch, "The vehicle autopilot"):
    observe()                     one launch: every row's record
    policy                        torch, on the same stream, observation_tensor() -> command_tensor()
    run(repeat)                   `repeat` x (one controller launch, one tick)
    end_step(auto_restart=True)   who is done and why, then the restart of exactly those scenes -- cursors included
Nothing crosses to the host inside the loop.  At the end the autopilot's records say how the traffic fared: how many cars are held
up by a pedestrian, how many by another car.
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

CIRCUIT = 12.0           # half the side of the square the cars drive round, metres
TRAFFIC = dict(v0=5.0, T=1.2, s0=2.0, acc=1.5, dec=2.0, brake=6.0, half_width=1.3, front=2.5, look=25.0, reach=3.0, ped_margin=0.5,
               max_turn=0.08)


def circuits(scenes):
    """Per scene, per vehicle: a closed square path about the crowd's centre of mass, each car starting at another corner."""
    corners = CIRCUIT * np.array([[1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0], [1.0, -1.0]])
    out = []
    for sc in scenes:
        mid = np.asarray(sc["loc"], dtype=np.float64)[:, :2].mean(axis=0)
        out.append([mid + np.roll(corners, -(k % 4), axis=0) for k in range(len(sc["dynamic_obstacles"]))])
    return out


def run(B=256, steps=200, repeat=4, max_age=150, device=0, quiet=False):
    import torch
    from carla_social_force_model_amd import autopilot, scenarios
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
        b.set_vehicle_autopilot(circuits(scenes), loop=True, **TRAFFIC)   # the traffic drives itself from here on
        b.snapshot()                                                    # the reset state of every scene, cursors included
        obs, cmd, rec = b.observation_tensor(), b.command_tensor(), b.episode_tensor()
        agents = torch.arange(B, device=obs.device) * N_B
        tally = torch.zeros(2, dtype=torch.int64, device=obs.device)   # episodes ended, of them at the goal
        for step in range(steps):
            b.observe()
            cmd[agents, 0:2] = policy(obs[agents])
            b.run(repeat)
            b.end_step(auto_restart=True)
            ended = rec[:, EP_DONE] != 0
            tally[0] += ended.sum()
            tally[1] += (ended & ((rec[:, EP_REASON].to(torch.int32) & REASON_ARRIVED) != 0)).sum()
        episodes, arrivals = (int(v) for v in tally.cpu())
        records = np.concatenate([r for _, r in b.vehicle_autopilot()])   # the one copy of the traffic's records, after the loop
        behind_ped = int((records[:, 1] == autopilot.KIND_PEDESTRIAN).sum())
        behind_car = int((records[:, 1] == autopilot.KIND_VEHICLE).sum())
        if not quiet:
            print(f"{B} scenes of {N_B}, {steps} steps of {repeat} ticks: {episodes} episodes ended, {arrivals} of them at the goal; "
                  f"of {len(records)} autopiloted cars {behind_ped} follow a pedestrian and {behind_car} another car, mean speed "
                  f"{float(records[:, 6].mean()):.2f} m/s")
        return episodes, arrivals, behind_ped, behind_car
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
