"""Pedestrian spawners for batched scenes: a mirror of the reference's PedSpawner without CARLA, the expansion of spawners into
the rows and spawn schedule a batch takes (``SfmBatch.upload`` + ``set_modes`` + ``set_spawns``), and a NumPy twin of the birth
rule the batch kernel applies every tick.

The reference describes a crowd as spawners (pedestrian_spawner.py): each releases ``quantity`` pedestrians, at most one per tick,
whenever ``next_spawn_time <= sim_time``, and pushes ``next_spawn_time`` on by ``spawn_interval`` per release.  A batch scene
keeps a fixed set of rows -- everyone who will ever walk in it -- so a spawner becomes ``quantity`` consecutive rows: row k's
``spawn_time`` is the value ``next_spawn_time`` has when pedestrian k is released, and ``chain = 1`` on all but the first makes
row k wait for row k - 1 to be born in an earlier tick, which is the one-release-per-tick rule (it matters when the interval is
shorter than the step length, or the spawner starts behind the clock).  Pure NumPy; nothing here touches the GPU.
"""
from __future__ import annotations

import numpy as np

from .host_state import PedMode, PedModeManager

MODE_UNBORN = 254                # SFM_MODE_UNBORN: what SfmBatch.modes() reports while a row waits for its spawn time


class PedSpawner:
    """Everything needed to release one or more pedestrians from one spawn point (the reference's PedSpawner,
    pedestrian_spawner.py:194-263, same constructor arguments and attributes).  The initial velocity points from the spawn
    location to the first waypoint in the plane: ``speed * (cos a, sin a, 0)``, a = atan2 of that direction -- what the
    reference's round trip through a CARLA transform (yaw in degrees, forward vector) amounts to."""

    def __init__(self, spawn_location, waypoints, crossing_road_bools, speed, blueprint, quantity, spawn_time, spawn_interval,
                 crossing_speed_factor, crossing_safety_margin):
        self.spawn_location = np.asarray(spawn_location, dtype=np.float64)
        self.target_speed = speed
        self.blueprint = blueprint
        self.quantity = quantity
        self.spawn_interval = spawn_interval
        self.next_spawn_time = spawn_time
        self.crossing_speed_factor = crossing_speed_factor
        self.crossing_safety_margin = crossing_safety_margin
        self.initial_mode = PedMode.CROSSING_ROAD if crossing_road_bools[0] else PedMode.WALKING_SIDEWALK
        waypoints = np.asarray(waypoints, dtype=np.float64)
        if waypoints.ndim > 1:
            self.first_waypoint = waypoints[0]
            self.remaining_waypoint_tuples = list(zip(waypoints[1:].tolist(), list(crossing_road_bools[1:])))
        else:                                                         # a single waypoint given flat
            self.first_waypoint = waypoints
            self.remaining_waypoint_tuples = []
        d = self.first_waypoint - self.spawn_location
        a = float(np.arctan2(d[1], d[0]))
        self.velocity = np.array([np.cos(a), np.sin(a), 0.0]) * speed

    def ready_to_spawn(self, sim_time):
        """True once per call while the spawner is due; each True pushes ``next_spawn_time`` on by one interval."""
        if self.next_spawn_time <= sim_time:
            self.next_spawn_time += self.spawn_interval
            return True
        return False

    def generate_ped_state(self, name, carla_id, radius):
        """(initial pedestrian state as PedState.add_pedestrian takes it, remaining (waypoint, crossing_road) tuples)."""
        mode = PedModeManager(name, self.target_speed, self.initial_mode, self.crossing_speed_factor, self.crossing_safety_margin)
        return ((name, carla_id, self.spawn_location, self.velocity, self.first_waypoint, mode, radius, self.target_speed),
                self.remaining_waypoint_tuples)


def release_times(spawner):
    """The value ``next_spawn_time`` has at each of the spawner's ``quantity`` releases, accumulated in float64 by repeated
    addition like ``ready_to_spawn`` does (the spawner itself is left alone)."""
    out = np.zeros(int(spawner.quantity), dtype=np.float64)
    t = float(spawner.next_spawn_time)
    for k in range(out.shape[0]):
        out[k] = t
        t += spawner.spawn_interval
    return out


def births(born, spawn_time, chain, now):
    """The batch's birth rule for ONE scene and one tick: ``born`` (N,) bool before the tick, ``spawn_time`` (N,), ``chain``
    (N,) 0 / 1, ``now`` the scene's clock before the tick -> born after it.  An unborn row i is born iff ``spawn_time[i] <= now``
    in float32 and, if ``chain[i]``, row i - 1 was born BEFORE this tick.  Start from ``born`` all False at the clock the schedule
    is set on: the rows the batch keeps live at that moment (due, ``chain = 0``) are the ones this rule lets in in the first tick,
    and a row chained to one of them waits one tick more -- as the reference's spawn manager, which runs at the top of every tick,
    releases them."""
    born = np.asarray(born, dtype=bool).reshape(-1)
    st = np.asarray(spawn_time, dtype=np.float32).reshape(-1)
    ch = np.asarray(chain).reshape(-1).astype(bool)
    if not (born.shape == st.shape == ch.shape):
        raise ValueError(f"births: born {born.shape}, spawn_time {st.shape} and chain {ch.shape} differ in length")
    if ch.size and ch[0]:
        raise ValueError("births: chain must be 0 on the scene's first row")
    before = np.concatenate([[True], born[:-1]]) if born.size else born
    return born | ((st <= np.float32(now)) & (~ch | before))


def birth_ticks(spawn_time, chain, clock0, dt, ticks):
    """The tick in which each row of one scene is born over ``ticks`` ticks of a float32 clock that starts at ``clock0`` and
    advances by ``dt`` per tick like the batch's, the schedule being set at ``clock0``: 0 = in the first tick (which includes
    the rows the batch keeps live when the schedule is set), ``ticks`` = not born inside the run.
    Returns (tick (N,) int64, clock before that tick (N,) float32, NaN where unborn)."""
    st = np.asarray(spawn_time, dtype=np.float32).reshape(-1)
    now = np.float32(clock0)
    born = np.zeros(st.shape, bool)
    tick = np.full(st.shape, int(ticks), dtype=np.int64)
    when = np.full(st.shape, np.nan, dtype=np.float32)
    for t in range(int(ticks)):
        new = births(born, st, chain, now) & ~born
        tick[new] = t
        when[new] = now
        born |= new
        now = np.float32(now + np.float32(dt))
    return tick, when


def scene_from_spawners(spawners, radius=0.3, present=(), present_queues=None):
    """Spawners -> the rows of one batch scene, in release order: spawner by spawner, ``quantity`` rows each.

    ``radius``: one value, or one per spawner.  ``present``: pedestrians already there at tick 0, as initial pedestrian states
    (name, id, location, velocity, first waypoint, PedModeManager, radius, target speed -- what ``generate_ped_state`` returns
    first), with ``present_queues`` their remaining (waypoint, crossing_road) lists; they come first, with ``spawn_time = -inf``.

    Returns (scene, plan, schedule, managers): ``scene`` holds loc, vel, waypoint (N,3), target_speed, radius (N,) for a scene dict
    (add the geometry keys), ``plan`` the mode plan ``SfmBatch.set_modes`` takes (``plan_from_managers``), ``schedule`` the
    ``spawn_time`` float32 / ``chain`` uint8 dict ``SfmBatch.set_spawns`` takes, ``managers`` the mode objects (for a host loop).
    The spawners are not advanced."""
    from .batch import plan_from_managers
    spawners, present = list(spawners), list(present)
    rad = np.broadcast_to(np.asarray(radius, dtype=np.float64).reshape(-1), (len(spawners),)) if spawners else np.zeros(0)
    if present_queues is None:
        present_queues = [[] for _ in present]
    if len(present_queues) != len(present):
        raise ValueError(f"{len(present_queues)} present_queues for {len(present)} present pedestrians")
    loc, vel, wp, ts, rr, managers, queues, times, chain = [], [], [], [], [], [], [], [], []

    def row(state, queue, t, c):
        _, _, x, v, w, mode, r, speed = state
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        loc.append(np.asarray(x, dtype=np.float64)); vel.append(np.asarray(v, dtype=np.float64))
        wp.append(np.array([w[0], w[1], w[2] if w.size > 2 else 0.0]))
        ts.append(float(speed)); rr.append(float(r)); managers.append(mode); queues.append(list(queue))
        times.append(t); chain.append(c)

    for state, q in zip(present, present_queues):
        row(state, q, -np.inf, 0)
    for s, sp in enumerate(spawners):
        for k, t in enumerate(release_times(sp)):
            state, rem = sp.generate_ped_state(f"ped_{len(loc)}", len(loc), rad[s])
            row(state, rem, t, 1 if k else 0)
    n = len(loc)
    scene = {"loc": np.array(loc, dtype=np.float64).reshape(n, 3), "vel": np.array(vel, dtype=np.float64).reshape(n, 3),
             "waypoint": np.array(wp, dtype=np.float64).reshape(n, 3), "target_speed": np.array(ts, dtype=np.float64),
             "radius": np.array(rr, dtype=np.float64)}
    schedule = {"spawn_time": np.asarray(times, dtype=np.float64).astype(np.float32), "chain": np.asarray(chain, dtype=np.uint8)}
    return scene, plan_from_managers(managers, queues), schedule, managers
