"""Scripted vehicle spawners for batched scenes: a mirror of the reference's VehicleSpawner without CARLA, and the expansion of
spawners into the tracks a batch takes (``SfmBatch.set_vehicle_tracks``).

The reference's scripted traffic (vehicle_spawner.py, run_simulation.py): a spawner holds ``trajectory`` (locations), ``headings``
(radians) and ``speeds``, one entry per tick, and releases ``quantity`` vehicles, at most one per tick, whenever
``next_spawn_time <= sim_time``, pushing ``next_spawn_time`` on by ``spawn_interval`` per release.  The list handling, line by line:

* the constructor pops ``trajectory[0]`` / ``headings[0]`` for the spawn transform (vehicle_spawner.py:197-198) and keeps
  ``speeds[1:]`` (:164);
* a released vehicle gets the remaining entries as its own list of transforms (:140-143);
* in the very tick of its release, after the spawn managers and before anything looks at the traffic, every scripted vehicle is
  teleported to the next entry of its list with that entry's heading and ``forward * speed`` (run_simulation.py:52-62,
  carla_simulation.py:107-111) -- so what the pedestrians of the release tick see is entry 1, never entry 0;
* in the tick in which its list is empty the vehicle is destroyed (run_simulation.py:63-66).

So a spawner of L entries gives each vehicle the L - 1 keyframes ``1 .. L-1``, seen in the release tick and the L - 2 ticks after
it, and the vehicle is gone in tick ``release + L - 1``.

One quirk is documented and NOT reproduced: with ``quantity > 1`` the reference hands every vehicle of a spawner the SAME
``speeds`` list object (vehicle_spawner.py:144), so the first vehicle's pops eat the speeds of the later ones (which then run out
of speeds while they still have transforms).  The mirror gives each vehicle its own copy.

Only the scripted keys are taken.  ``auto_pilot`` (traffic manager or BehaviorAgent), ``spawn_point`` (a map's recommended spawn
points) and ``destination`` need the simulator and its map: they are refused.  Pure NumPy; nothing here touches the GPU.
(Traffic that drives itself on a batch -- a path, a gap to the car in front, braking for walkers -- is ``SfmBatch.set_vehicle_autopilot``.)
"""
from __future__ import annotations

import numpy as np


class VehicleSpawner:
    """Everything needed to release one or more scripted vehicles (the reference's VehicleSpawner, vehicle_spawner.py:149-203,
    scripted arguments only; same attribute names).  ``trajectory`` (L,2|3), ``headings`` (L,) radians, ``speeds`` (L,), L >= 2."""

    def __init__(self, trajectory, headings, speeds, quantity=1, spawn_time=0.0, spawn_interval=5.0, auto_pilot=False,
                 spawn_point=None, destination=None):
        if auto_pilot:
            raise ValueError("auto_pilot vehicles are driven by the simulator's traffic manager or a BehaviorAgent, which this "
                             "mirror does not have: give a scripted trajectory (auto_pilot = false)")
        if spawn_point is not None or destination is not None:
            raise ValueError("spawn_point and destination index the simulator map's recommended spawn points, which this mirror "
                             "does not have: give the spawn transform as the first entry of trajectory / headings")
        trajectory = [np.asarray(p, dtype=np.float64).reshape(-1) for p in trajectory]
        headings = [float(h) for h in np.asarray(headings, dtype=np.float64).reshape(-1)]
        speeds = [float(v) for v in np.asarray(speeds, dtype=np.float64).reshape(-1)]
        if not (len(trajectory) == len(headings) == len(speeds)):
            raise ValueError(f"trajectory ({len(trajectory)}), headings ({len(headings)}) and speeds ({len(speeds)}) must have "
                             "one entry per tick each")
        if len(trajectory) < 2:
            raise ValueError("a scripted vehicle needs at least 2 entries: the spawn transform and one keyframe (the reference "
                             "destroys a vehicle with an empty list in its release tick)")
        if any(p.size not in (2, 3) for p in trajectory):
            raise ValueError("trajectory entries must have 2 or 3 coordinates")
        if int(quantity) != quantity or quantity < 0:
            raise ValueError(f"quantity must be a whole number >= 0, got {quantity!r}")
        self.auto_pilot = False
        self.spawn_point = None
        self.destination = None
        self.spawn_location = trajectory[0]                  # generate_carla_spawn_transform: trajectory.pop(0), headings.pop(0)
        self.spawn_heading = headings[0]
        self.trajectory = trajectory[1:]
        self.headings = headings[1:]
        self.speeds = speeds[1:]                             # vehicle_spawner.py:164
        self.quantity = int(quantity)
        self.spawn_interval = spawn_interval
        self.next_spawn_time = spawn_time

    def ready_to_spawn(self, sim_time):
        """True once per call while the spawner is due; each True pushes ``next_spawn_time`` on by one interval."""
        if self.next_spawn_time <= sim_time:
            self.next_spawn_time += self.spawn_interval
            return True
        return False


def release_times(spawner):
    """The value ``next_spawn_time`` has at each of the spawner's ``quantity`` releases, accumulated in float64 by repeated
    ``+=`` like ``ready_to_spawn`` does (the spawner itself is left alone)."""
    out = np.zeros(int(spawner.quantity), dtype=np.float64)
    t = float(spawner.next_spawn_time)
    for k in range(out.shape[0]):
        out[k] = t
        t += spawner.spawn_interval
    return out


def first_ticks(times, dt, sim_time0=0.0):
    """Release ticks of ONE spawner on a float32 clock ``sim_time0, + dt, + dt, ...`` (the clock of ``spawner.birth_ticks`` and of
    the batch's scenes): vehicle k is released in the first tick whose clock value ``now`` has ``float32(times[k]) <= now`` and
    that lies after vehicle k - 1's tick (one release per spawner per tick).  A time at or behind ``sim_time0`` gives tick 0 for
    the first vehicle; ticks are never negative here (``tracks_from_spawners`` makes them so by skipping keyframes)."""
    out = []
    now, tick = np.float32(sim_time0), 0
    step = np.float32(dt)
    if not step > 0:
        raise ValueError("dt must be > 0")
    for t in np.asarray(times, dtype=np.float64).astype(np.float32):
        if not np.isfinite(t):
            raise ValueError("spawn times must be finite")
        while not t <= now:
            now = np.float32(now + step)
            tick += 1
        out.append(tick)
        now = np.float32(now + step)                         # the next vehicle of this spawner waits for a later tick
        tick += 1
    return out


def tracks_from_spawners(spawners, dt, sim_time0=0.0, elapsed_ticks=0):
    """Spawners -> one track per vehicle, spawner by spawner, ``quantity`` tracks each: the list ``SfmBatch.set_vehicle_tracks``
    takes for one scene whose vehicles are given in that order.  Keyframes are entries 1 .. L-1 of the spawner's lists (see the
    module docstring), ``first_tick`` the release tick on the float32 clock ``sim_time0, + dt, ...`` (``first_ticks``: the rule and
    the clock of ``spawner.birth_ticks``, so pedestrians and vehicles with the same ``spawn_time`` enter in the same tick).

    ``elapsed_ticks``: ticks the scenario has already run when the tracks are set; ``sim_time0`` is the clock of tick 0 of the
    scenario, the tracks' tick 0 is its tick ``elapsed_ticks``, and a vehicle released before that gets a negative
    ``first_tick`` (it is met under way, or already gone).  The spawners are not advanced."""
    tracks = []
    for sp in spawners:
        xy = np.array([p[:2] for p in sp.trajectory], dtype=np.float64).reshape(-1, 2)
        yaw = np.array(sp.headings, dtype=np.float64)
        speed = np.array(sp.speeds, dtype=np.float64)          # (each vehicle its own copy: the quirk of :144 is not reproduced)
        for tick in first_ticks(release_times(sp), dt, sim_time0):
            tracks.append({"xy": xy.copy(), "yaw": yaw.copy(), "speed": speed.copy(), "first_tick": int(tick) - int(elapsed_ticks)})
    return tracks
