#!/usr/bin/env python3
"""Golden spawner traces from the REFERENCE's PedSpawner (pedestrian_spawner.py), for tests/test_batch_spawns_host.py.

The reference module imports carla and path_planner, which only its PedSpawnManager needs; PedSpawner itself uses a Transform's
location / rotation and ``get_forward_vector``.  Stand-in modules written here supply exactly that (and the one GraphType
attribute the module reads at import), so the reference's own class runs without CARLA.  Build-container only:
``SFM_REFERENCE=<checkout> make_golden_spawn.py`` writes tests/golden/spawn/spawn_schedule.npz (a directory of its own: the
files directly under tests/golden/ are force cases, and the force tests run every one of them); ``--inputs-only --out DIR`` writes
only the inputs (no upstream code runs), which the drift guard compares with the committed file.

Per case: one spawner driven over a float32 clock (clock0, + dt per tick in float32, like a batch scene's) the way
PedSpawnManager.tick drives it: ``ready_to_spawn(sim_time)`` while quantity > 0, quantity -= 1 on a release.  Recorded: the release
flag and ``next_spawn_time`` after every tick, and the fields of ``generate_ped_state``."""
import argparse
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (spawn_location, waypoints, crossing_road_bools, speed, quantity, spawn_time, spawn_interval, crossing_speed_factor,
#  crossing_safety_margin, dt, clock0, ticks)
CASES = [
    # interval above the step length
    ([1.0, 2.0, 0.0], [[4.0, 6.0, 0.0], [8.0, 6.0, 0.0], [8.0, 12.0, 0.0]], [False, True, False], 1.2, 5, 0.3, 3.0, 1.5, 1.5, 0.05, 0.0, 300),
    # interval below the step length: one release per tick
    ([-3.0, 0.5, 0.0], [[-3.0, 9.0, 0.0], [2.0, 9.0, 0.0]], [False, True], 1.4, 9, 0.3, 0.02, 1.5, 1.5, 0.05, 0.0, 30),
    # spawn_time before the clock's start: a backlog, one release per tick until it is caught up
    ([10.0, -4.0, 0.0], [[2.0, -4.0, 0.0], [2.0, 3.0, 0.0]], [True, False], 1.0, 6, 1.0, 0.5, 1.3, 2.0, 0.05, 2.5, 60),
    # the first leg crosses a road; interval a non-representable multiple of the step
    ([0.0, 0.0, 0.0], [[-5.0, -5.0, 0.0], [-9.0, -5.0, 0.0]], [True, True], 1.6, 7, 0.1, 0.13, 2.0, -1.0, 0.04, 0.0, 60),
    # a single waypoint, given flat
    ([2.5, 2.5, 0.0], [2.5, -7.5, 0.0], [False], 0.9, 3, 0.0, 0.2, 1.5, 1.5, 0.05, 0.0, 20),
    # interval equal to the step length, behind the clock, more pedestrians than ticks
    ([7.0, 1.0, 0.0], [[7.0, 5.0, 0.0], [3.0, 5.0, 0.0]], [False, True], 1.1, 12, -0.2, 0.05, 1.5, 1.5, 0.05, 0.0, 10),
]
T_MAX = max(c[-1] for c in CASES)


def inputs():
    """The cases as flat arrays (ragged waypoint lists as CSR)."""
    off = np.zeros(len(CASES) + 1, dtype=np.int64)
    wps, cross, flat = [], [], []
    for k, c in enumerate(CASES):
        w = np.asarray(c[1], dtype=np.float64)
        flat.append(w.ndim == 1)
        w = w.reshape(-1, 3)
        wps.append(w)
        cross.extend(bool(x) for x in c[2])
        off[k + 1] = off[k] + len(w)
    return dict(in_loc=np.array([c[0] for c in CASES], dtype=np.float64), in_wp_off=off, in_wp=np.concatenate(wps),
                in_cross=np.array(cross, dtype=bool), in_flat=np.array(flat, dtype=bool),
                in_scalars=np.array([c[3:11] for c in CASES], dtype=np.float64),   # speed, quantity, spawn_time, interval, factor, margin, dt, clock0
                in_ticks=np.array([c[11] for c in CASES], dtype=np.int64))


def stand_ins():
    """carla and path_planner as far as pedestrian_spawner.py touches them outside PedSpawnManager."""
    carla = types.ModuleType("carla")

    class Location:
        def __init__(self, x=0.0, y=0.0, z=0.0):
            self.x, self.y, self.z = x, y, z

    class Rotation:
        def __init__(self, pitch=0.0, yaw=0.0, roll=0.0):
            self.pitch, self.yaw, self.roll = pitch, yaw, roll

    class Vector3D(Location):
        pass

    class Transform:
        def __init__(self):
            self.location, self.rotation = Location(), Rotation()

        def get_forward_vector(self):
            yaw, pitch = math.radians(self.rotation.yaw), math.radians(self.rotation.pitch)
            return Vector3D(math.cos(pitch) * math.cos(yaw), math.cos(pitch) * math.sin(yaw), math.sin(pitch))

    carla.Location, carla.Rotation, carla.Vector3D, carla.Transform = Location, Rotation, Vector3D, Transform
    planner = types.ModuleType("path_planner")
    planner.PedPathPlanner = object
    planner.GraphType = types.SimpleNamespace(JAYWALKING_AT_JUNCTION=0)
    sys.modules["carla"], sys.modules["path_planner"] = carla, planner


def reference_outputs(ref_dir, d):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref_dir)
    stand_ins()
    import pedestrian_spawner as ps                                      # (reference)
    C = len(CASES)
    release = np.zeros((C, T_MAX), dtype=np.uint8)
    nxt = np.full((C, T_MAX), np.nan)
    vel, first, mode4 = np.zeros((C, 3)), np.zeros((C, 3)), np.zeros((C, 4))
    initial_mode, speed, radius = np.zeros(C, dtype=np.int64), np.zeros(C), np.zeros(C)
    rem_off = np.zeros(C + 1, dtype=np.int64)
    rem_wp, rem_cross = [], []
    for k in range(C):
        w = d["in_wp"][d["in_wp_off"][k]:d["in_wp_off"][k + 1]]
        bools = [bool(x) for x in d["in_cross"][d["in_wp_off"][k]:d["in_wp_off"][k + 1]]]
        sp_, qty, t0, interval, factor, margin, dt, clock0 = d["in_scalars"][k]
        sp = ps.PedSpawner(d["in_loc"][k].copy(), w[0].copy() if d["in_flat"][k] else w.copy(), bools, float(sp_), None, int(qty),
                           float(t0), float(interval), float(factor), float(margin))
        now = np.float32(clock0)
        for t in range(int(d["in_ticks"][k])):
            if sp.quantity > 0 and sp.ready_to_spawn(float(now)):       # PedSpawnManager.tick
                release[k, t] = 1
                sp.quantity -= 1
            nxt[k, t] = sp.next_spawn_time
            now = np.float32(now + np.float32(dt))
        state, rem = sp.generate_ped_state(f"ped_{k}", 100 + k, 0.25 + 0.05 * k)
        vel[k], first[k], radius[k], speed[k] = state[3], state[4], state[6], state[7]
        initial_mode[k] = int(sp.initial_mode)
        m = state[5]
        mode4[k] = (int(m.current_mode), m.target_speed, m.crossing_speed, m.crossing_safety_margin)
        rem_off[k + 1] = rem_off[k] + len(rem)
        rem_wp.extend(r[0] for r in rem)
        rem_cross.extend(bool(r[1]) for r in rem)
    return dict(ref_release=release, ref_next_spawn_time=nxt, ref_velocity=vel, ref_first_waypoint=first, ref_mode=mode4,
                ref_initial_mode=initial_mode, ref_target_speed=speed, ref_radius=radius, ref_rem_off=rem_off,
                ref_rem_wp=np.asarray(rem_wp, dtype=np.float64).reshape(-1, 3), ref_rem_cross=np.asarray(rem_cross, dtype=bool))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "spawn"))
    a = ap.parse_args()
    d = inputs()
    if not a.inputs_only:
        ref = os.environ.get("SFM_REFERENCE", "")
        if not os.path.isdir(ref):
            print("SFM_REFERENCE does not name a reference checkout -- nothing to do")
            return
        d.update(reference_outputs(ref, d))
    np.savez_compressed(os.path.join(a.out, "spawn_schedule.npz"), **d)
    print("wrote spawn_schedule.npz:", len(CASES), "spawners;", "inputs only" if a.inputs_only else
          f"releases per case {d['ref_release'].sum(axis=1).tolist()}")


if __name__ == "__main__":
    main()
