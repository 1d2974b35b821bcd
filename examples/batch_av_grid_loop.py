"""examples/batch_av_lidar_loop.py with a bird's-eye raster in place of the lidar: the ego vehicle's policy is a small conv net over
the grid around its own vehicle, nothing on the host.

    python examples/batch_av_grid_loop.py [--scenes 256] [--steps 200] [--repeat 2]

The scenes, the crossing pedestrians and the unicycle are those of batch_av_loop.py.  What differs is the sensor: a window of
GU x GV cells in the vehicle's heading frame that looks further ahead than behind (carla_social_force_model_amd.batch, "Bird's-eye
grids around the vehicles"): pedestrians and their relative velocities, kerbs, parked obstacles and the other vehicles per cell.
The vehicle's own ring is left out, so the vehicle does not see itself as an obstacle.
    grid_vehicles()          one launch: every gridded vehicle's (8, GV, GU) raster
    policy                   torch, on the same stream, vehicle_grid_tensor() -> vehicle_command_tensor(): a fixed 3 x 3 convolution
                             spreads the occupancy, the nearest occupied column of the corridor ahead sets the speed, the goal
                             entry of the last record the turn
    run(repeat)              `repeat` ticks on the held command, one launch per tick
    observe_vehicles()       one launch: clearance and goal entry, for the reward and the episode's end only
    restart_device(done)     one launch: exactly those scenes back to the snapshot
Nothing crosses to the host inside the loop: no `.cpu()`, no mask download.  Needs an MI355X; importing this file does not."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import batch_av_loop as AV  # noqa: E402  (the scenes and the constants of the loop without a raster)

GU, GV = 48, 20              # cells forward and sideways
CELL = 0.5                   # metres per cell
CENTRE = (8.0, 0.0)          # the middle of the window: 4 m behind the vehicle's centre to 20 m ahead
LANE = 2.5                   # half width of the corridor the vehicle keeps free, metres
FRONT = 2.4                  # the front of the box, metres ahead of the centre
CRUISE = AV.CRUISE


def policy(grid, goal=None):
    """A small conv policy on the raster (M, 8, GV, GU) -> commands (M, 3) = (speed, cos, sin of the turn).  Occupancy is the sum of
    the pedestrian, static-obstacle and other-vehicle counts; one 3 x 3 convolution of ones spreads it by a cell (a pedestrian half
    a cell outside the corridor still counts); the nearest occupied column ahead of the bumper, inside the corridor, sets the speed
    by batch_av_loop.py's rule; ``goal`` (M, 2), the goal entry in the heading frame, sets the turn (None: straight on)."""
    import torch
    import torch.nn.functional as F
    occ = (grid[:, 0] + grid[:, 4] + grid[:, 5]).unsqueeze(1)
    spread = F.conv2d(occ, torch.ones(1, 1, 3, 3, device=grid.device, dtype=grid.dtype), padding=1)[:, 0]
    along = (torch.arange(GU, device=grid.device, dtype=grid.dtype) + 0.5 - 0.5 * GU) * CELL + CENTRE[0]      # cell centres, metres
    across = (torch.arange(GV, device=grid.device, dtype=grid.dtype) + 0.5 - 0.5 * GV) * CELL + CENTRE[1]
    corridor = (across.abs() < LANE)[None, :, None] & (along > FRONT)[None, None, :]
    ahead = (spread > 0.0) & corridor
    gap = torch.where(ahead, along[None, None, :].expand_as(spread), torch.full_like(spread, 1.0e3)).amin(dim=(1, 2))
    speed = (CRUISE * ((gap - 4.0) / 8.0)).clamp(0.0, CRUISE)
    turn = torch.zeros_like(speed) if goal is None else torch.atan2(goal[:, 1], goal[:, 0]).clamp(-0.02, 0.02)   # per tick
    return torch.stack((speed, torch.cos(turn), torch.sin(turn)), dim=1)


def run(B=256, steps=200, repeat=2, device=0, quiet=False):
    import torch
    from carla_social_force_model_amd import scenarios
    from carla_social_force_model_amd.batch import DRIVE_UNICYCLE, SfmBatch
    from carla_social_force_model_amd.config import default_sfm_config

    scenes, plans = AV.make_scenes(B)
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), AV.DT, device=device, B=B)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)          # torch and the batch on one stream: launches and reads are ordered
        b.upload(scenes, device_vehicles=True)
        b.set_modes(plans, despawn_on_arrival=False, sim_time0=0.0, arrive_thresholds=1.0, scenes=scenes)
        b.set_vehicle_driving(DRIVE_UNICYCLE, np.float32([CRUISE, 1.0, 0.0]))
        b.set_vehicle_observation(AV.K, AV.SENSE_RANGE, frame=1, goals=np.float32(AV.GOAL))
        b.set_vehicle_grid(CELL, GU, GV, frame=1, centre=CENTRE)
        b.snapshot()                                                    # the reset state of every scene
        obs, raster, cmd = b.vehicle_observation_tensor(), b.vehicle_grid_tensor(), b.vehicle_command_tensor()
        ret = torch.zeros(B, device=obs.device)
        tally = torch.zeros(3, dtype=torch.int64, device=obs.device)   # episodes ended, at the goal, by a collision
        age = torch.zeros(B, dtype=torch.int32, device=obs.device)
        b.observe_vehicles()
        for step in range(steps):
            b.grid_vehicles()
            cmd[:, 0:3] = policy(raster, obs[:, 0:2])                   # (the goal entry is as old as the last observe_vehicles())
            b.run(repeat)
            b.observe_vehicles()
            goal_d2 = obs[:, 0] * obs[:, 0] + obs[:, 1] * obs[:, 1]
            hit = obs[:, 8] < AV.HIT_RADIUS * AV.HIT_RADIUS             # clear_d2: ring to the nearest live pedestrian
            near = (obs[:, 8] < 1.0) & ~hit
            arrived = goal_d2 < AV.GOAL_RADIUS * AV.GOAL_RADIUS
            age += 1
            late = age >= 400
            ret += obs[:, 15] * (AV.DT * repeat) - 0.1 * near.float() - 10.0 * hit.float() + 10.0 * arrived.float()
            done = hit | arrived | late
            tally += torch.stack((done.sum(), arrived.sum(), hit.sum()))
            b.restart_device(done)                                      # a torch bool mask, on the device
            age = torch.where(done, torch.zeros_like(age), age)
        episodes, arrivals, hits = (int(v) for v in tally.cpu())        # the one copy, after the loop
        if not quiet:
            print(f"{B} scenes of {AV.N_B} pedestrians and one ego vehicle with a {GU} x {GV} raster, {steps} steps of {repeat} ticks: "
                  f"{episodes} episodes ended, {arrivals} at the goal, {hits} by a collision; mean return {float(ret.mean()):.2f}")
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
