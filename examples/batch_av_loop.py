"""A driving loop with nothing on the host: an ego vehicle per scene, driven by a torch policy against a crowd that crosses its road.

    python examples/batch_av_loop.py [--scenes 256] [--steps 200] [--repeat 2]

Every scene is a straight road along x with a sidewalk on either side.  Its pedestrians wait at the kerb in CHECKING_TRAFFIC and
cross when the reference's gap acceptance lets them -- which looks at the ego vehicle's velocity, i.e. at what the policy commanded a
tick earlier.  The ego vehicle (vehicle 0 of its scene, the only one) is a unicycle (carla_social_force_model_amd.batch, "Driven
vehicles"): the policy outputs a signed speed and a turn per step, cos and sin of the turn are taken in torch, and the three numbers go
into the vehicle command buffer.
    observe_vehicles()       one launch: every vehicle's record (heading frame) -- goal, speed, nearest pedestrians, clearance
    policy                   torch, on the same stream, vehicle_observation_tensor() -> vehicle_command_tensor()
    run(repeat)              `repeat` ticks on the held command (the turn applies every tick), one launch per tick
    reward, done             torch, from the clearance clear_d2 and the goal entry of the record
    restart_device(done)     one launch: exactly those scenes back to the snapshot -- pedestrians, modes, vehicle pose AND heading
Nothing crosses to the host inside the loop: no `.cpu()`, no mask download.  Needs an MI355X; importing this file does not."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_B = 16                 # pedestrians per scene
K = 4                    # pedestrian slots of the vehicle's record
SENSE_RANGE = 12.0       # metres
DT = 0.05
CRUISE = 6.0             # m/s
GOAL = (25.0, 0.0)
GOAL_RADIUS = 2.0
HIT_RADIUS = 0.4         # a ring point closer than this to a pedestrian is a collision
EXTENT = (2.4, 1.0)


def make_scenes(B, seed=0):
    """B scenes and their mode plans: pedestrians at both kerbs (y = +-4) spread along the road, each about to cross."""
    from carla_social_force_model_amd import scenarios
    from carla_social_force_model_amd.batch import plan_from_managers
    from carla_social_force_model_amd.host_state import PedMode, PedModeManager
    rng = np.random.default_rng(seed)
    local = scenarios.ring_local_offsets(*EXTENT)
    scenes, plans = [], []
    for _ in range(B):
        side = np.where(np.arange(N_B) % 2 == 0, 1.0, -1.0)
        x = rng.uniform(-10.0, 20.0, N_B)
        loc = np.column_stack((x, 4.0 * side + rng.uniform(-0.3, 0.3, N_B), np.zeros(N_B)))
        wp = np.column_stack((x + rng.uniform(-1.0, 1.0, N_B), -4.0 * side, np.zeros(N_B)))
        ts = rng.uniform(1.0, 1.4, N_B)
        c = np.array([-20.0 + rng.uniform(-2.0, 2.0), rng.uniform(-0.5, 0.5)])
        scenes.append({"loc": loc, "vel": np.zeros((N_B, 3)), "waypoint": wp, "target_speed": ts, "radius": np.full(N_B, 0.3),
                       "borders": [], "border_centers": np.zeros((0, 2)), "border_lengths": np.zeros(0), "static_obstacles": [],
                       "dynamic_obstacles": [(c, scenarios.place_ring_f32(c, 0.0, local))], "dynamic_vel": np.array([[CRUISE, 0.0]]),
                       "dynamic_yaw": np.zeros(1), "dynamic_extent": np.array([EXTENT])})
        managers, queues = [], []
        for i in range(N_B):
            m = PedModeManager(f"ped_{i}", float(ts[i]), PedMode.WALKING_SIDEWALK, 1.5, 1.0)
            m.set_mode(PedMode.CROSSING_ROAD)                          # from the sidewalk: CHECKING_TRAFFIC first
            managers.append(m)
            queues.append([(np.array([wp[i, 0] + 6.0, wp[i, 1] - 2.0 * side[i], 0.0]), False)])
        plans.append(plan_from_managers(managers, queues))
    return scenes, plans


def policy(obs):
    """A small hand-written policy on the heading-frame record (B, 16 + 4K) -> (speed, turn) per vehicle: steer towards the goal,
    slow down for the nearest pedestrian ahead, stop when it is close."""
    import torch
    goal = obs[:, 0:2]
    turn = torch.atan2(goal[:, 1], goal[:, 0]).clamp(-0.02, 0.02)          # per tick; the goal entry is in the heading frame
    slots = obs[:, 16:16 + 4 * K].reshape(-1, K, 4)
    filled = torch.arange(K, device=obs.device)[None, :] < obs[:, 7:8]
    ahead = filled & (slots[:, :, 0] > 0.0) & (slots[:, :, 1].abs() < 2.5)
    gap = torch.where(ahead, slots[:, :, 0], torch.full_like(slots[:, :, 0], 1.0e3)).min(dim=1).values
    speed = (CRUISE * ((gap - 4.0) / 8.0)).clamp(0.0, CRUISE)
    return speed, turn


def run(B=256, steps=200, repeat=2, device=0, quiet=False):
    import torch
    from carla_social_force_model_amd import scenarios
    from carla_social_force_model_amd.batch import DRIVE_UNICYCLE, SfmBatch
    from carla_social_force_model_amd.config import default_sfm_config

    scenes, plans = make_scenes(B)
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, device=device, B=B)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)          # torch and the batch on one stream: launches and reads are ordered
        b.upload(scenes, device_vehicles=True)
        b.set_modes(plans, despawn_on_arrival=False, sim_time0=0.0, arrive_thresholds=1.0, scenes=scenes)
        b.set_vehicle_driving(DRIVE_UNICYCLE, np.float32([CRUISE, 1.0, 0.0]))
        b.set_vehicle_observation(K, SENSE_RANGE, frame=1, goals=np.float32(GOAL))
        b.snapshot()                                                    # the reset state of every scene
        obs, cmd = b.vehicle_observation_tensor(), b.vehicle_command_tensor()
        ret = torch.zeros(B, device=obs.device)
        tally = torch.zeros(3, dtype=torch.int64, device=obs.device)   # episodes ended, at the goal, by a collision
        age = torch.zeros(B, dtype=torch.int32, device=obs.device)
        for step in range(steps):
            b.observe_vehicles()
            speed, turn = policy(obs)
            cmd[:, 0], cmd[:, 1], cmd[:, 2] = speed, torch.cos(turn), torch.sin(turn)
            b.run(repeat)
            b.observe_vehicles()
            goal_d2 = obs[:, 0] * obs[:, 0] + obs[:, 1] * obs[:, 1]
            hit = obs[:, 8] < HIT_RADIUS * HIT_RADIUS                   # clear_d2: ring to the nearest live pedestrian
            near = (obs[:, 8] < 1.0) & ~hit
            arrived = goal_d2 < GOAL_RADIUS * GOAL_RADIUS
            age += 1
            late = age >= 400
            ret += obs[:, 15] * (DT * repeat) - 0.1 * near.float() - 10.0 * hit.float() + 10.0 * arrived.float()
            done = hit | arrived | late
            tally += torch.stack((done.sum(), arrived.sum(), hit.sum()))
            b.restart_device(done)                                      # a torch bool mask, on the device
            age = torch.where(done, torch.zeros_like(age), age)
        episodes, arrivals, hits = (int(v) for v in tally.cpu())        # the one copy, after the loop
        if not quiet:
            print(f"{B} scenes of {N_B} pedestrians and one ego vehicle, {steps} steps of {repeat} ticks: {episodes} episodes ended, "
                  f"{arrivals} at the goal, {hits} by a collision; mean return {float(ret.mean()):.2f}")
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
