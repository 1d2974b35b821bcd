"""examples/batch_av_loop.py with a lidar: the ego vehicle's policy reads a range scan cast from its own bumper, nothing on the host.

    python examples/batch_av_lidar_loop.py [--scenes 256] [--steps 200] [--repeat 2] [--rays 128]

The scenes, the crossing pedestrians and the unicycle are those of batch_av_loop.py.  What differs is the sensor: a forward fan of
rays from a mount at the front of the vehicle, in the vehicle's heading frame (carla_social_force_model_amd.batch, "Range scans from
the vehicles").  The vehicle's own ring is left out of its scan, so the sensor may sit anywhere inside the body.
    scan_vehicles()          one launch: every vehicle's R ranges and kinds
    policy                   torch, on the same stream, vehicle_scan_tensor() -> vehicle_command_tensor(): the ranges set the speed,
                             the goal entry of the last record the turn
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

import batch_av_loop as AV  # noqa: E402  (the scenes and the constants of the loop without a lidar)

RAYS = 128
FAN = 5.0 * np.pi / 6.0      # the fan's half angle: 150 degrees to either side, so that it sees what walks beside the bonnet
MAX_RANGE = 20.0             # metres
MOUNT = (2.4, 0.0)           # the front of the box, on its axis
LANE = 2.5                   # half width of the corridor the vehicle keeps free, metres
CRUISE = AV.CRUISE


def fan_angles(R):
    """R angles from -FAN to FAN; an odd R has a ray straight ahead."""
    return np.linspace(-FAN, FAN, int(R))


def policy(ranges, dirs, goal=None):
    """A small hand-written policy on the heading-frame ranges (M, R) and the ray directions (R, 2) -> commands (M, 3) = (speed, cos,
    sin of the turn): the nearest hit inside the corridor ahead of the vehicle's centre sets the speed (batch_av_loop.py's rule on
    what the rays met: ``along`` is measured from the sensor, MOUNT[0] in front of the centre); ``goal`` (M, 2), the goal entry in
    the heading frame, sets the turn (None: straight on)."""
    import torch
    hit = ranges < MAX_RANGE
    along, across = ranges * dirs[None, :, 0] + MOUNT[0], ranges * dirs[None, :, 1]
    ahead = hit & (along > 0.0) & (across.abs() < LANE)
    gap = torch.where(ahead, along, torch.full_like(along, 1.0e3)).min(dim=1).values
    speed = (CRUISE * ((gap - 4.0) / 8.0)).clamp(0.0, CRUISE)
    turn = torch.zeros_like(speed) if goal is None else torch.atan2(goal[:, 1], goal[:, 0]).clamp(-0.02, 0.02)   # per tick
    return torch.stack((speed, torch.cos(turn), torch.sin(turn)), dim=1)


def run(B=256, steps=200, repeat=2, rays=RAYS, device=0, quiet=False):
    import torch
    from carla_social_force_model_amd import scan, scenarios
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
        b.set_vehicle_scan(MAX_RANGE, ped_radius=0.3, angles=fan_angles(rays), frame=1, mount=MOUNT)
        b.snapshot()                                                    # the reset state of every scene
        obs, lidar, cmd = b.vehicle_observation_tensor(), b.vehicle_scan_tensor(), b.vehicle_command_tensor()
        dirs = torch.as_tensor(np.stack(scan.ray_directions(fan_angles(rays), scan.MAX_VEHICLE_SCAN_RAYS), axis=1), device=obs.device)
        ret = torch.zeros(B, device=obs.device)
        tally = torch.zeros(3, dtype=torch.int64, device=obs.device)   # episodes ended, at the goal, by a collision
        age = torch.zeros(B, dtype=torch.int32, device=obs.device)
        b.observe_vehicles()
        for step in range(steps):
            b.scan_vehicles()
            cmd[:, 0:3] = policy(lidar[:, :rays], dirs, obs[:, 0:2])       # (the goal entry is as old as the last observe_vehicles())
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
            print(f"{B} scenes of {AV.N_B} pedestrians and one ego vehicle with {rays} rays, {steps} steps of {repeat} ticks: "
                  f"{episodes} episodes ended, {arrivals} at the goal, {hits} by a collision; mean return {float(ret.mean()):.2f}")
        return episodes, arrivals, hits
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--rays", type=int, default=RAYS)
    args = ap.parse_args()
    run(args.scenes, args.steps, args.repeat, args.rays)


if __name__ == "__main__":
    main()
