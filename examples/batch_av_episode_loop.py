"""The driving loop of batch_av_loop.py with the episode ends decided on the device: no geometry in torch, nothing on the host.

    python examples/batch_av_episode_loop.py [--scenes 256] [--steps 200] [--repeat 2]

The scenes, the crowd and the policy are batch_av_loop.py's.  What differs is everything behind the ticks: there the loop assembled
`done`, an age counter and the reward from slot 8 of the vehicle observation -- the clearance of the sampled RING, which lets a
pedestrian stand against the flank between two samples and calls one 40 cm in front of a corner a hit, and which knows nothing of
walls or other cars.  Here
    end_vehicle_step(auto_restart=True)      one launch decides every ego vehicle's fate on exact gaps to its oriented BOX (arrived,
                                             time limit, pedestrian, vehicle, wall) and leaves what a reward is made of in the
                                             vehicle record; a second launch restarts the scenes that are done
    reward                                   torch, from slots 3 .. 7 of the record: progress towards the goal, the gaps, the reason
The loop keeps no age tensor and assembles no `done`.  Nothing crosses to the host inside it.  Needs an MI355X; importing this file
does not."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_av_loop import CRUISE, DT, EXTENT, GOAL, GOAL_RADIUS, K, N_B, SENSE_RANGE, make_scenes, policy  # noqa: E402

HIT_RADIUS = 0.3         # a pedestrian's centre closer than this to the BODY is a collision (a pedestrian's radius)
NEAR = 1.0               # metres: closer than this costs a little
MAX_STEPS = 400


def run(B=256, steps=200, repeat=2, device=0, quiet=False):
    import torch
    from carla_social_force_model_amd import scenarios
    from carla_social_force_model_amd.batch import (DRIVE_UNICYCLE, EP_GOAL_D2, EP_PED_GAP2, EP_PREV_GOAL_D2, EP_REASON, REASON_ARRIVED,
                                                    REASON_PED_HIT, SfmBatch)
    from carla_social_force_model_amd.config import default_sfm_config

    scenes, plans = make_scenes(B)
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, device=device, B=B)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)          # torch and the batch on one stream: launches and reads are ordered
        b.upload(scenes, device_vehicles=True)
        b.set_modes(plans, despawn_on_arrival=False, sim_time0=0.0, arrive_thresholds=1.0, scenes=scenes)
        b.set_vehicle_driving(DRIVE_UNICYCLE, np.float32([CRUISE, 1.0, 0.0]))
        b.set_vehicle_observation(K, SENSE_RANGE, frame=1, goals=np.float32(GOAL))
        b.set_vehicle_episodes(True, goals=np.float32(GOAL), goal_radius=GOAL_RADIUS, ped_radius=HIT_RADIUS, veh_radius=0.0,
                               wall_radius=0.0, max_steps=MAX_STEPS)    # extents: the scenes' dynamic_extent
        b.snapshot()                                                    # the reset state of every scene
        obs, cmd, rec = b.vehicle_observation_tensor(), b.vehicle_command_tensor(), b.vehicle_episode_tensor()
        ret = torch.zeros(B, device=obs.device)
        tally = torch.zeros(3, dtype=torch.int64, device=obs.device)   # episodes ended, at the goal, by a collision
        for step in range(steps):
            b.observe_vehicles()
            speed, turn = policy(obs)
            cmd[:, 0], cmd[:, 1], cmd[:, 2] = speed, torch.cos(turn), torch.sin(turn)
            b.run(repeat)
            b.end_vehicle_step(auto_restart=True)                       # fate and restart on the device; the record keeps the terminal values
            reason = rec[:, EP_REASON].to(torch.int32)
            arrived, hit = (reason & REASON_ARRIVED) != 0, (reason & REASON_PED_HIT) != 0
            progress = rec[:, EP_PREV_GOAL_D2].sqrt() - rec[:, EP_GOAL_D2].sqrt()          # metres gained towards the goal
            near = (rec[:, EP_PED_GAP2] < NEAR * NEAR) & ~hit
            ret += progress - 0.1 * near.float() - 10.0 * hit.float() + 10.0 * arrived.float()
            tally += torch.stack(((reason != 0).sum(), arrived.sum(), hit.sum()))
        episodes, arrivals, hits = (int(v) for v in tally.cpu())        # the one copy, after the loop
        if not quiet:
            print(f"{B} scenes of {N_B} pedestrians and one ego vehicle, {steps} steps of {repeat} ticks: {episodes} episodes ended, "
                  f"{arrivals} at the goal, {hits} by a collision with the body; mean return {float(ret.mean()):.2f}")
        return episodes, arrivals, hits
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=2)
    args = ap.parse_args()
    run(args.scenes, args.steps, args.repeat)


if __name__ == "__main__":
    main()
