"""Deterministic synthetic crowds + geometry in the reference's own input formats.

The reference needs a CARLA server to produce its inputs (pedestrian_spawner.py, obstacles.py); the
BASELINE configs are CARLA-free, so this module generates inputs of the same *shape*:

* pedestrians: the 8-field spawn tuple of pedestrian_spawner.py:230-243
  (name, id, loc3, vel3, first_waypoint3, mode, radius, target_speed); target speed 1.2 +- 0.1
  (pedestrian_spawner.py:73,146-147);
* borders: straight polylines sampled every 0.1 m with ``center = line[len//2]`` and
  ``section_length = len(line) * resolution`` (obstacles.py:344-355);
* static / dynamic obstacles: ``(center, ring)`` with an ellipse ring scaled by sqrt(2) and
  ``max(6, int((2*ex + 2*ey) / resolution))`` samples (obstacles.py:269-281, 297-329).

Every coordinate is rounded to fp32 before it is stored in float64: the
device state is fp32, so parity scenarios must be fp32-representable.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

RESOLUTION = 0.1  # m, obstacles.py:25 default


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@dataclass
class Scenario:
    loc: np.ndarray            # (N,3) f64, fp32-representable
    vel: np.ndarray            # (N,3)
    waypoint: np.ndarray       # (N,3)
    target_speed: np.ndarray   # (N,)
    radius: np.ndarray         # (N,)
    mode: np.ndarray           # (N,) int, PedMode values
    borders: list = field(default_factory=list)            # list of (P_k,2)
    border_centers: np.ndarray = None                      # (K,2)
    border_lengths: np.ndarray = None                      # (K,)
    static_obstacles: list = field(default_factory=list)   # list of (center(2), ring(P,2))
    dynamic_obstacles: list = field(default_factory=list)
    dynamic_vel: np.ndarray = None                         # (M,2)
    dynamic_yaw: np.ndarray = None                         # (M,)
    dynamic_extent: np.ndarray = None                      # (M,2)
    world_side: float = 0.0
    seed: int = 0

    @property
    def n(self):
        return self.loc.shape[0]

    def section_info(self):
        """border_section_info in the form BorderForce indexes it (forces.py:130-132): an object array
        K x [center(2), length] (a ragged list only converts on NumPy < 1.24)."""
        info = np.empty((len(self.borders), 2), dtype=object)
        for k in range(len(self.borders)):
            info[k, 0] = self.border_centers[k]
            info[k, 1] = float(self.border_lengths[k])
        return info


def straight_border(start, end, resolution=RESOLUTION):
    """One config-style border (obstacles.py:344-355)."""
    start = np.asarray(start, dtype=np.float64)
    end = np.asarray(end, dtype=np.float64)
    samples = int(np.linalg.norm(end - start) / resolution)
    line = _f32(np.column_stack((np.linspace(start[0], end[0], samples),
                                 np.linspace(start[1], end[1], samples))))
    center = line[len(line) // 2]
    return line, center, len(line) * resolution


def ellipse_ring(center, yaw, ex, ey, resolution=RESOLUTION, scale=np.sqrt(2.0)):
    """Ring of border points around an oriented box (obstacles.py:269-281), yaw in radians."""
    samples = max(6, int((2.0 * ex + 2.0 * ey) / resolution))
    th = 2.0 * np.pi * np.arange(samples) / samples
    px, py = ex * np.cos(th) * scale, ey * np.sin(th) * scale
    c, s = np.cos(yaw), np.sin(yaw)
    ring = np.column_stack((center[0] + c * px - s * py, center[1] + s * px + c * py))
    return _f32(ring)


def ring_local_offsets(ex, ey, resolution=RESOLUTION, scale=np.sqrt(2.0)):
    """The ellipse of generate_ellipse_border before the vehicle transform (obstacles.py:269-281), fp32."""
    samples = max(6, int((2.0 * ex + 2.0 * ey) / resolution))
    th = 2.0 * np.pi * np.arange(samples) / samples
    return _f32(np.column_stack((ex * np.cos(th) * scale, ey * np.sin(th) * scale)))


def place_ring_f32(center, yaw, local):
    """p = c + R(yaw) u evaluated the way the device does (fp32, fused multiply-adds): the host-side twin of
    sfm_dynamic_boxes_kernel, so CPU checks see bit-identical ring points."""
    c32 = np.asarray(center, dtype=np.float32).astype(np.float64)
    cs, sn = np.float64(np.float32(np.cos(yaw))), np.float64(np.float32(np.sin(yaw)))
    u = np.asarray(local, dtype=np.float32).astype(np.float64)
    fma = lambda a, b, c: np.float32(a * b + c).astype(np.float64)      # product of two fp32 is exact in f64
    px = fma(cs, u[:, 0], fma(-sn, u[:, 1], c32[0]))
    py = fma(sn, u[:, 0], fma(cs, u[:, 1], c32[1]))
    return np.column_stack((px, py))


def advance_center_f32(center, vel, dt):
    c = np.asarray(center, dtype=np.float32).astype(np.float64)
    v = np.asarray(vel, dtype=np.float32).astype(np.float64)
    return np.float32(np.float64(np.float32(dt)) * v + c).astype(np.float64)


def make_crowd(n, seed, density=0.25, jitter=0.8, z_spread=0.0):
    """Jittered-grid crowd.  Returns (loc, vel, waypoint, target_speed, radius,
    world_side)."""
    rng = np.random.default_rng(seed)
    g = int(np.ceil(np.sqrt(n)))
    cell = 1.0 / np.sqrt(density)
    side = g * cell
    k = np.arange(n)
    cx = (k % g + 0.5) * cell
    cy = (k // g + 0.5) * cell
    loc = np.zeros((n, 3))
    loc[:, 0] = cx + rng.uniform(-jitter, jitter, n)
    loc[:, 1] = cy + rng.uniform(-jitter, jitter, n)
    if z_spread:
        loc[:, 2] = rng.uniform(0.0, z_spread, n)
    wp = np.zeros((n, 3))
    wp[:, :2] = rng.uniform(0.0, side, (n, 2))
    to = wp[:, :2] - loc[:, :2]
    ang = np.arctan2(to[:, 1], to[:, 0]) + rng.normal(0.0, 0.3, n)
    speed = rng.uniform(0.6, 1.4, n)
    vel = np.zeros((n, 3))
    vel[:, 0] = speed * np.cos(ang)
    vel[:, 1] = speed * np.sin(ang)
    if z_spread:
        vel[:, 2] = rng.normal(0.0, 0.05, n)
    tspeed = 1.2 + rng.uniform(-0.1, 0.1, n)
    radius = np.full(n, 0.3)
    return _f32(loc), _f32(vel), _f32(wp), _f32(tspeed), _f32(radius), float(np.float32(side))


def make_scenario(n, seed, n_borders=0, n_static=0, n_dynamic=0, z_spread=0.0, density=0.25,
                  border_len=(10.0, 40.0), modes=None):
    """Full synthetic scenario: crowd + K_b borders + M_s static + M_d dynamic obstacles."""
    loc, vel, wp, tspeed, radius, side = make_crowd(n, seed, density, z_spread=z_spread)
    rng = np.random.default_rng(seed + 7919)
    sc = Scenario(loc=loc, vel=vel, waypoint=wp, target_speed=tspeed, radius=radius,
                  mode=np.ones(n, dtype=np.int64) if modes is None else np.asarray(modes, dtype=np.int64),
                  world_side=side, seed=seed)
    cents, lens = [], []
    for _ in range(n_borders):
        o = rng.uniform(0.0, side, 2)
        h = rng.uniform(0.0, 2.0 * np.pi)
        ln = rng.uniform(*border_len)
        line, c, sl = straight_border(o, o + ln * np.array([np.cos(h), np.sin(h)]))
        sc.borders.append(line)
        cents.append(c)
        lens.append(sl)
    sc.border_centers = np.array(cents).reshape(-1, 2)
    sc.border_lengths = np.array(lens, dtype=np.float64)
    for _ in range(n_static):
        c = _f32(rng.uniform(0.0, side, 2))
        ex, ey = rng.uniform(0.2, 1.5, 2)
        sc.static_obstacles.append((c, ellipse_ring(c, rng.uniform(0.0, 2.0 * np.pi), ex, ey)))
    yaws, vels, exts = [], [], []
    for _ in range(n_dynamic):
        c = _f32(rng.uniform(0.0, side, 2))
        yaw = rng.uniform(0.0, 2.0 * np.pi)
        sp = rng.uniform(0.0, 14.0)
        sc.dynamic_obstacles.append((c, place_ring_f32(c, yaw, ring_local_offsets(2.4, 1.0))))
        yaws.append(yaw)
        vels.append(_f32([sp * np.cos(yaw), sp * np.sin(yaw)]))
        exts.append([2.4, 1.0])
    sc.dynamic_vel = np.array(vels, dtype=np.float64).reshape(-1, 2)
    sc.dynamic_yaw = np.array(yaws, dtype=np.float64)
    sc.dynamic_extent = np.array(exts, dtype=np.float64).reshape(-1, 2)
    return sc


def advance_dynamic(sc: Scenario, dt):
    """Move the vehicles one step and rebuild their rings (what the simulator + get_dynamic_obstacles do per
    tick, obstacles.py:297-329), in the device's fp32 arithmetic."""
    new = []
    for k, (c, _) in enumerate(sc.dynamic_obstacles):
        c2 = advance_center_f32(c, sc.dynamic_vel[k], dt)
        new.append((c2, place_ring_f32(c2, sc.dynamic_yaw[k], ring_local_offsets(*sc.dynamic_extent[k]))))
    sc.dynamic_obstacles = new
    return sc


def _accessors(sc):
    if isinstance(sc, dict):
        return sc.get, sc.__setitem__
    return (lambda k, d=None: getattr(sc, k, d)), (lambda k, v: setattr(sc, k, v))


def track_present(track, tau):
    """Does tick ``tau`` see the vehicle of ``track`` (None: untracked, always there)?  0 <= tau - first_tick < L."""
    if track is None:
        return True
    return 0 <= int(tau) - int(track["first_tick"]) < len(np.asarray(track["yaw"]).reshape(-1))


def place_tracked(sc, tracks, tau, dt=None):
    """The host twin of the batch's vehicle tracks for ONE scene (a Scenario or a scene dict; ``tracks``: None or one entry per
    vehicle, each None or a track dict as ``batch.pack_tracks`` takes it): sets ``dynamic_obstacles``, ``dynamic_vel`` and
    ``dynamic_yaw`` to what integrating tick ``tau`` after ``set_vehicle_tracks`` sees, bit for bit what the device holds, and
    ``dynamic_present`` (M,) bool.

    A tracked vehicle that is present (0 <= tau - first_tick < L) is AT keyframe j = tau - first_tick: centre the float32 of
    ``xy[j]``, velocity the float32 of the float64 products ``speed[j] * (cos, sin)(yaw[j])``, ring ``place_ring_f32`` at
    ``yaw[j]`` -- a teleport, the step length plays no part.  Otherwise it is absent: centre and every ring point +inf, velocity 0
    (its squared distance to anyone is +inf, which fails every strict-< cull; speed 0 never makes gap acceptance refuse).  An
    untracked vehicle follows ``advance_dynamic``'s rule: with ``dt`` given it moves one step of ``dt`` (the call that goes from
    tick tau - 1 to tick tau), without it stays (tau = 0, or a tick that did not integrate).  Returns ``sc``."""
    get, put = _accessors(sc)
    dyn = list(get("dynamic_obstacles") or [])
    M = len(dyn)
    tracks = [None] * M if tracks is None else list(tracks)
    if len(tracks) != M:
        raise ValueError(f"{len(tracks)} tracks for {M} vehicles")
    vel = get("dynamic_vel")
    vel = np.zeros((M, 2)) if vel is None else np.array(vel, dtype=np.float64).reshape(M, 2)
    yaws = np.array(get("dynamic_yaw"), dtype=np.float64).reshape(M)
    ext = np.asarray(get("dynamic_extent"), dtype=np.float64).reshape(M, 2)
    present = np.ones(M, dtype=bool)
    new = []
    for k, (c, ring) in enumerate(dyn):
        tr = tracks[k]
        local = ring_local_offsets(*ext[k])
        if tr is None:
            if dt is not None:
                c = advance_center_f32(c, vel[k], dt)
            new.append((np.asarray(c, dtype=np.float64), place_ring_f32(c, yaws[k], local)))
            continue
        j = int(tau) - int(tr["first_tick"])
        if track_present(tr, tau):
            yaw = float(np.asarray(tr["yaw"], dtype=np.float64).reshape(-1)[j])
            sp = float(np.asarray(tr["speed"], dtype=np.float64).reshape(-1)[j])
            c = _f32(np.asarray(tr["xy"], dtype=np.float64).reshape(-1, 2)[j])
            vel[k] = _f32([sp * np.cos(yaw), sp * np.sin(yaw)])
            yaws[k] = yaw
            new.append((c, place_ring_f32(c, yaw, local)))
        else:
            present[k] = False
            vel[k] = 0.0
            new.append((np.full(2, np.inf), np.full((len(local), 2), np.inf)))
    put("dynamic_obstacles", new)
    put("dynamic_vel", vel)
    put("dynamic_yaw", yaws)
    put("dynamic_present", present)
    return sc


def vehicle_headings(sc):
    """The vehicles' headings (M,2) float32 {cos, sin} as the device holds them: ``dynamic_heading`` once ``drive_vehicles`` has
    stored it, else the fp32 cos / sin of the float64 ``dynamic_yaw`` (what ``batch.pack_boxes`` sends)."""
    get, _ = _accessors(sc)
    h = get("dynamic_heading")
    if h is not None:
        return np.array(h, dtype=np.float32).reshape(-1, 2)
    yaw = np.asarray(get("dynamic_yaw") if get("dynamic_yaw") is not None else [], dtype=np.float64).reshape(-1)
    return np.column_stack((np.cos(yaw), np.sin(yaw))).astype(np.float32)


def place_ring_heading_f32(center, heading, local):
    """``place_ring_f32`` from a stored fp32 heading {cos, sin}: p = (fmaf(hx, ux, fmaf(-hy, uy, cx)), fmaf(hy, ux, fmaf(hx, uy, cy)))
    with exact fused multiply-adds (``scan._fma32``), float64 values of fp32 numbers."""
    from .scan import _fma32
    c = np.asarray(center, dtype=np.float32)
    h = np.asarray(heading, dtype=np.float32)
    u = np.asarray(local, dtype=np.float32).reshape(-1, 2)
    px = _fma32(h[0], u[:, 0], _fma32(-h[1], u[:, 1], c[0]))
    py = _fma32(h[1], u[:, 0], _fma32(h[0], u[:, 1], c[1]))
    return np.column_stack((px, py)).astype(np.float64)


def drive_command(kind, command, heading):
    """The rule of a driven vehicle (drive_vehicle in sfm_interaction.h; include/sfm_hip.h states it) without the move: kind 1 or 2,
    the fp32 command (a, b, c) and heading (hx, hy) -> (heading' (2,), velocity' (2,)) float32, every line one correctly rounded
    fp32 operation or an exact fmaf."""
    from .scan import _fma32
    a, b, c = (np.float32(v) for v in command)
    hx, hy = (np.float32(v) for v in heading)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if int(kind) == 1:
            s2 = _fma32(a, a, b * b)
            if s2 > 0:
                s = np.sqrt(s2)
                hx, hy = a / s, b / s
            return np.array([hx, hy], np.float32), np.array([a, b], np.float32)
        gx = _fma32(b, hx, -(c * hy))
        gy = _fma32(c, hx, b * hy)
        n2 = _fma32(gx, gx, gy * gy)
        if n2 > 0:
            n = np.sqrt(n2)
            hx, hy = gx / n, gy / n
        return np.array([hx, hy], np.float32), np.array([a * hx, a * hy], np.float32)


def drive_vehicles(sc, kinds, commands, dt, tracks=None, tau=None):
    """The host twin of the batch's driven vehicles for ONE scene (a Scenario or a scene dict) and ONE integrating tick of step
    ``dt``: moves ``dynamic_obstacles`` (centres and rings), ``dynamic_vel`` and the headings ``dynamic_heading`` (M,2) float32 the
    way the device does, bit for bit (include/sfm_hip.h states the rule; every operation is fp32, fused multiply-adds are exact).

    ``kinds`` (M,) or one value: 1 velocity, 2 unicycle, anything else not driven; ``commands`` (M,3) or one (3,) command: (a, b, c).
    A vehicle that is not driven does what it does without driving: with ``tracks`` (one entry per vehicle, None or a track dict)
    and ``tau`` (the tick this call arrives at), a vehicle that has keyframes is placed by ``place_tracked``'s rule -- its stored
    heading stays what it was -- and any other moves by ``dt`` times its velocity, its ring placed at its stored heading.  A driven
    vehicle ignores its keyframes; one whose centre is not finite stays absent (centre and ring +inf, velocity 0, heading kept).
    Sets ``dynamic_present`` (M,) bool and keeps ``dynamic_yaw`` in step with the headings (float64, for readers; the device holds
    no angle).  Returns ``sc``."""
    from .scan import _fma32
    get, put = _accessors(sc)
    dyn = list(get("dynamic_obstacles") or [])
    M = len(dyn)
    kd = np.broadcast_to(np.asarray(kinds, dtype=np.float64), (M,)) if np.ndim(kinds) == 0 else np.asarray(kinds, dtype=np.float64).reshape(M)
    cmd = np.asarray(commands, dtype=np.float32)
    cmd = np.broadcast_to(cmd, (M, 3)) if cmd.ndim == 1 else cmd.reshape(M, 3)
    tracks = [None] * M if tracks is None else list(tracks)
    if len(tracks) != M:
        raise ValueError(f"{len(tracks)} tracks for {M} vehicles")
    vel = get("dynamic_vel")
    vel = np.zeros((M, 2), np.float32) if vel is None else np.array(vel, dtype=np.float64).reshape(M, 2).astype(np.float32)
    head = vehicle_headings(sc).copy()
    ext = np.asarray(get("dynamic_extent"), dtype=np.float64).reshape(M, 2)
    yaws = np.array(get("dynamic_yaw"), dtype=np.float64).reshape(M)
    dt32 = np.float32(dt)
    tracked = None
    if any(t is not None for t in tracks):                              # the keyframe rule, taken from its one definition
        if tau is None:
            raise ValueError("drive_vehicles: tracks need tau, the tick this call arrives at")
        tracked = place_tracked({"dynamic_obstacles": dyn, "dynamic_vel": vel.astype(np.float64), "dynamic_yaw": yaws.copy(),
                                 "dynamic_extent": ext}, tracks, tau, dt)
    present = np.ones(M, dtype=bool)
    new = []
    for k, (c, _) in enumerate(dyn):
        local = ring_local_offsets(*ext[k])
        c32 = np.asarray(c, dtype=np.float64).astype(np.float32)
        if kd[k] in (1.0, 2.0):
            h2, v2 = drive_command(kd[k], cmd[k], head[k])
            if np.isfinite(c32).all():
                head[k], vel[k] = h2, v2
                c2 = np.array([_fma32(dt32, v2[0], c32[0]), _fma32(dt32, v2[1], c32[1])], np.float32)
                new.append((c2.astype(np.float64), place_ring_heading_f32(c2, h2, local)))
                yaws[k] = np.arctan2(np.float64(h2[1]), np.float64(h2[0]))
            else:
                present[k] = False
                vel[k] = 0.0
                new.append((np.full(2, np.inf), np.full((len(local), 2), np.inf)))
        elif tracks[k] is not None:
            new.append(tracked["dynamic_obstacles"][k])
            vel[k] = tracked["dynamic_vel"][k]
            yaws[k] = tracked["dynamic_yaw"][k]
            present[k] = tracked["dynamic_present"][k]
        else:
            c2 = np.array([_fma32(dt32, vel[k, 0], c32[0]), _fma32(dt32, vel[k, 1], c32[1])], np.float32)
            new.append((c2.astype(np.float64), place_ring_heading_f32(c2, head[k], local)))
    put("dynamic_obstacles", new)
    put("dynamic_vel", vel.astype(np.float64))
    put("dynamic_yaw", yaws)
    put("dynamic_heading", head)
    put("dynamic_present", present)
    return sc


def make_track_plan(sc, seed, ticks, dt=0.05, max_speed=1.4):
    """A synthetic track plan for one scene (a Scenario or a scene dict), the recipe of the batch track tests: every vehicle drives
    a gentle arc (constant turn rate, up to +-0.6 rad over the run) that passes through the crowd's centre of mass half-way; the
    keyframes are dt apart at the keyframe speeds, so position and speed agree.  Vehicle 0 brakes linearly to speed 0, stands for
    about a tenth of the run and pulls away again; vehicle k enters at tick 3 k (staggered entries; vehicle 0 at tick -2, already
    under way); the last vehicle's list ends at about two thirds of the run (an exit inside ``ticks``), the others' at ``ticks``
    or later.  Speeds stay <= ``max_speed``.  Returns the list ``SfmBatch.set_vehicle_tracks`` takes for the scene."""
    get, _ = _accessors(sc)
    M = len(get("dynamic_obstacles") or [])
    loc = np.asarray(get("loc"), dtype=np.float64).reshape(-1, 3)
    mid = loc[:, :2].mean(axis=0) if len(loc) else np.zeros(2)
    rng = np.random.default_rng(seed)
    ticks = int(ticks)
    tracks = []
    for k in range(M):
        first = -2 if k == 0 else 3 * k
        last = ticks + 2 if k < M - 1 or M == 1 else max(first + 1, (2 * ticks) // 3)
        if M == 1:
            last = max(first + 1, (2 * ticks) // 3)
        L = max(1, last - first)
        speed = np.full(L, rng.uniform(0.6, 1.0) * max_speed)
        if k == 0 and L >= 8:
            a, b = L // 4, L // 4 + max(1, L // 10)
            ramp = max(2, L // 8)
            speed[a - ramp:a] = speed[0] * np.linspace(1.0, 0.0, ramp, endpoint=False)
            speed[a:b] = 0.0
            speed[b:b + ramp] = speed[0] * np.linspace(0.0, 1.0, ramp, endpoint=False)
        yaw0 = rng.uniform(-np.pi, np.pi)
        yaw = yaw0 + rng.uniform(-0.6, 0.6) * (np.arange(L) / max(L - 1, 1) - 0.5)
        step = speed[:, None] * dt * np.column_stack((np.cos(yaw), np.sin(yaw)))
        xy = np.cumsum(step, axis=0) - step
        xy += mid + rng.uniform(-1.0, 1.0, 2) - xy[L // 2]
        tracks.append({"xy": _f32(xy), "yaw": yaw, "speed": _f32(speed), "first_tick": int(first)})
    return tracks


def make_mode_plan(sc, seed, queue_len=3, idle_every=11, reckless_every=5):
    """A synthetic mode plan for one scene (a Scenario or a scene dict), the recipe of the device mode tests: every pedestrian a
    PedModeManager mirror walking the sidewalk (crossing speed 1.5 x target speed, safety margin 1 s), every ``reckless_every``-th
    (i % reckless_every == 0) crossing without looking (margin -1), every ``idle_every``-th (i % idle_every == 3) IDLE at t = 0
    (wakes up after 5 s); ``queue_len`` more waypoints each, steps of up to 4 m apart from the current one, every other leg crossing a
    road.  The scene's first waypoints are REWRITTEN in place to within 3 m of each pedestrian, so arrivals come early.  Returns
    (plan, managers): the plan as ``batch.plan_from_managers`` builds it, and the mirror objects themselves (for a host loop)."""
    from .batch import plan_from_managers
    from .host_state import PedMode, PedModeManager
    get = (lambda k: sc[k]) if isinstance(sc, dict) else (lambda k: getattr(sc, k))
    loc, wp, ts = get("loc"), get("waypoint"), get("target_speed")
    n = len(loc)
    rng = np.random.default_rng(seed)
    managers = []
    for i in range(n):
        m = PedModeManager(f"ped_{i}", float(ts[i]), PedMode.WALKING_SIDEWALK, 1.5,
                           -1.0 if reckless_every and i % reckless_every == 0 else 1.0)
        if idle_every and i % idle_every == 3:
            m.set_mode(PedMode.IDLE)
        managers.append(m)
    queues = []
    for i in range(n):
        p = np.asarray(wp[i], dtype=np.float64)[:2].copy()
        lst = []
        for k in range(queue_len):
            p = _f32(p + rng.uniform(-4.0, 4.0, 2))
            lst.append((np.array([p[0], p[1], 0.0]), bool((i + k) % 2)))
        queues.append(lst)
    if n:
        wp[:, :2] = _f32(np.asarray(loc, dtype=np.float64)[:, :2] + rng.uniform(-3.0, 3.0, (n, 2)))
    return plan_from_managers(managers, queues), managers


def make_spawn_plan(sc, seed, dt=0.05, t0=0.0, present=0.35, n_spawners=4, horizon=4.0):
    """A synthetic spawn schedule for one scene (a Scenario or a scene dict), the recipe of the batch spawn tests: the first
    ``present`` fraction of the rows is there from the start (``spawn_time = -inf``), the others are dealt in row order to
    ``n_spawners`` spawners of consecutive rows (``chain = 1`` on all but a spawner's first row).  Spawner 0 starts two steps
    BEHIND the clock ``t0`` with an interval of 0.4 steps (a backlog: one release per tick), spawner 1 has an interval of 0.4 steps
    too but starts inside the run, the others intervals of 2.5 to 6 steps; starts lie within ``horizon`` / 2 seconds of ``t0`` and
    intervals are scaled so that every spawner is done inside about ``horizon`` seconds.  Release times accumulate in float64 and are rounded to float32
    once, as ``spawner.scene_from_spawners`` does.  ``present = 0`` gives a scene in which everybody is unborn at first (spawner 0
    then starts inside the run as well).  The rows themselves (positions, waypoints, modes) are the scene's.  Returns the dict
    ``SfmBatch.set_spawns`` takes: ``spawn_time`` float32 (N,), ``chain`` uint8 (N,)."""
    get = (lambda k: sc[k]) if isinstance(sc, dict) else (lambda k: getattr(sc, k))
    n = len(get("loc"))
    rng = np.random.default_rng(seed)
    times = np.full(n, -np.inf)
    chain = np.zeros(n, dtype=np.uint8)
    n0 = min(n, int(round(present * n)))
    rest = n - n0
    groups = min(n_spawners, rest)
    bounds = n0 + (np.arange(groups + 1) * rest) // max(groups, 1)
    for g in range(groups):
        lo, hi = int(bounds[g]), int(bounds[g + 1])
        q = hi - lo
        if g == 0 and present > 0:
            start, interval = t0 - 2.0 * dt, 0.4 * dt
        else:
            start = t0 + float(rng.uniform(0.5 * dt, 0.5 * horizon))
            interval = 0.4 * dt if g == 1 else float(rng.uniform(2.5, 6.0)) * dt
            interval = min(interval, max(0.4 * dt, 0.5 * horizon / max(q, 1)))
        t = float(start)
        for i in range(lo, hi):
            times[i] = t
            t += interval
            chain[i] = 1 if i > lo else 0
    with np.errstate(over="ignore"):
        return {"spawn_time": times.astype(np.float32), "chain": chain}


# BASELINE.json configs: name -> (kwargs for make_scenario, enabled forces)
ALL_FORCES = ("acceleration_force", "pedestrian_force", "border_force",
              "static_obstacle_force", "dynamic_obstacle_force")
BASELINE_CONFIGS = {
    "c1": dict(n=64, seed=1001, n_borders=40, n_static=16, n_dynamic=4, forces=ALL_FORCES),
    "c2": dict(n=4096, seed=1002, forces=("acceleration_force", "pedestrian_force")),
    "c3": dict(n=16384, seed=1003, n_borders=2000, n_static=256, forces=ALL_FORCES),
    "c4": dict(n=65536, seed=1004, forces=("pedestrian_force",)),
    "c5": dict(n=262144, seed=1005, n_borders=2000, n_static=256, n_dynamic=512, forces=ALL_FORCES),
}


def baseline_scenario(name):
    kw = dict(BASELINE_CONFIGS[name])
    forces = kw.pop("forces")
    return make_scenario(**kw), forces


def respawn_vehicles_scene(chosen, snapshot, current):
    """One respawn of the chosen vehicles of one scene (sfm_batch_respawn_vehicles_device), the copy rule: a dict like ``current``
    in which every per-vehicle entry of a chosen vehicle is the snapshot's and everything else is ``current``'s, untouched.

    ``chosen``: (M,) nonzero = respawn the vehicle.  ``snapshot`` / ``current``: dicts of per-vehicle values as the snapshot holds
    them and as they are now -- ``centers`` (M,2), ``vel`` (M,2), ``headings`` (M,2), ``rings`` (a list of M (P_k,2) arrays) and,
    with an autopilot set, ``cursor`` (M,).  With ``age`` (M,) and ``prev`` (M,) in ``current`` (vehicle episodes are on) a chosen
    vehicle's episode starts over: age 0, prev NaN.  Keys that are not per vehicle pass through."""
    ch = np.asarray(chosen).reshape(-1) != 0
    out = dict(current)
    for key in ("centers", "vel", "headings", "cursor"):
        if key in current:
            a = np.array(current[key], copy=True)
            if a.shape[0] != ch.shape[0]:
                raise ValueError(f"{ch.shape[0]} choices for {a.shape[0]} vehicles ({key})")
            a[ch] = np.asarray(snapshot[key])[ch]
            out[key] = a
    if "rings" in current:
        out["rings"] = [np.array(snapshot["rings"][k] if ch[k] else current["rings"][k], copy=True) for k in range(ch.shape[0])]
    if "age" in current:
        age, prev = np.array(current["age"], dtype=np.int32, copy=True), np.array(current["prev"], dtype=np.float32, copy=True)
        age[ch], prev[ch] = 0, np.nan
        out["age"], out["prev"] = age, prev
    return out
