"""The vehicle autopilot of a batch on the host: packing for ``SfmBatch.set_vehicle_autopilot``, the NumPy twin of one controller
launch, and the float64 restatement of its speed rule.  Pure NumPy; importing it needs no GPU.

The rule is specified in include/sfm_hip.h (sfm_batch_set_vehicle_autopilot), operation by operation: every line is one correctly
rounded fp32 operation or an exact fmaf (``scan._fma32``), ``max(x, y)`` is ``x if x > y else y``.  ``autopilot_vehicle`` /
``autopilot_scene`` follow it line by line, so what they return is bit for bit what sfm_batch_vehicle_autopilot_kernel writes; the
move that follows is ``scenarios.drive_vehicles`` with the commands returned here (kind 2, the unicycle).

Each autopiloted vehicle follows a path of waypoints under a bounded turn per tick and sets its speed by the Intelligent Driver
Model (Treiber, Hennecke and Helbing 2000) against the nearest thing in its corridor: a pedestrian, a ring point of another vehicle,
or the end of its path.
"""
from __future__ import annotations

import numpy as np

from . import _args
from .scan import _fma32

SETTINGS = ("v0", "T", "s0", "acc", "dec", "brake", "half_width", "front", "look", "reach", "ped_margin")   # then cos_max, sin_max
N_SETTINGS = 13                          # SFM_BATCH_AUTOPILOT_SETTINGS
MAX_POINTS = 4096                        # SFM_BATCH_MAX_AUTOPILOT_POINTS
GAP_FLOOR = np.float32(0.01)             # SFM_AUTOPILOT_GAP_FLOOR
FLAG_LOOP, FLAG_IGNORE_WALKERS = 1, 2    # SFM_AUTOPILOT_*
KIND_NONE, KIND_PEDESTRIAN, KIND_VEHICLE, KIND_PATH_END = 0, 1, 2, 3
NEAR_LIMIT = np.float32(1.0e12)          # the live test of the observations: |x|, |y| < 1e12
DEFAULTS = dict(v0=8.0, T=1.0, s0=2.0, acc=1.5, dec=2.0, brake=6.0, half_width=1.2, front=2.5, look=40.0, reach=3.0,
                ped_margin=0.5, max_turn=0.05)
STOP = np.array([0.0, 1.0, 0.0, 2.0], np.float32)      # the command of an absent or finished vehicle
_STRICT = {"v0", "s0", "acc", "dec", "brake", "look", "reach"}


def pack_paths(paths, item_off):
    """Paths -> (path_off int32 [M+1], px, py float32 [P]).  ``item_off`` (B+1,): the vehicles' scene offsets
    (``batch.pack_boxes(...)[0]``).  ``paths``: a list with one entry per scene, each a list with one entry per vehicle of the scene:
    a (P_k, 2) array of waypoints, or None / an empty array (the vehicle is not autopiloted).  Raises ValueError on a shape that
    does not fit, a point that is not finite in float32, and a path of more than ``MAX_POINTS`` points."""
    io = np.asarray(item_off)
    B = len(io) - 1
    if len(paths) != B:
        raise ValueError(f"{len(paths)} entries of paths for {B} scenes")
    off, pts = [0], []
    for b, scene_paths in enumerate(paths):
        mb = int(io[b + 1] - io[b])
        scene_paths = [] if scene_paths is None else list(scene_paths)
        if len(scene_paths) != mb:
            raise ValueError(f"scene {b}: {len(scene_paths)} paths for {mb} vehicles")
        for k, p in enumerate(scene_paths):
            a = np.zeros((0, 2)) if p is None else np.asarray(p, dtype=np.float64)
            a = a.reshape(0, 2) if a.size == 0 else a
            if a.ndim != 2 or a.shape[1] != 2:
                raise ValueError(f"scene {b}, vehicle {k}: a path is (P, 2), got shape {a.shape}")
            if len(a) > MAX_POINTS:
                raise ValueError(f"scene {b}, vehicle {k}: {len(a)} path points; a path takes up to {MAX_POINTS}")
            with np.errstate(over="ignore"):
                a32 = a.astype(np.float32)
            if not np.isfinite(a32).all():
                raise ValueError(f"scene {b}, vehicle {k}: a path point is not finite in float32")
            pts.append(a32)
            off.append(off[-1] + len(a32))
    xy = np.concatenate(pts, axis=0) if pts else np.zeros((0, 2), np.float32)
    return np.asarray(off, np.int32), np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])


def _per_vehicle(v, name, item_off, kinds="iuf"):
    """One value, B values (one per scene, ``_args.per_scene``), a list of B entries each a value or (M_b,) values, or an ndarray (M,)
    over the vehicles of all scenes (an ndarray of M values is per vehicle also where M == B; a list never is) -> (M,) values."""
    io = np.asarray(item_off)
    B, M = len(io) - 1, int(io[-1])
    counts = np.diff(io).astype(np.int64)
    if isinstance(v, (list, tuple)) and len(v) == B and any(np.ndim(e) > 0 for e in v):
        parts = []
        for b, e in enumerate(v):
            a = np.asarray(e)
            if a.dtype.kind not in kinds:
                raise ValueError(f"scene {b}: {name} must be numbers, got {a.dtype}")
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] not in (1, int(counts[b]))):
                raise ValueError(f"scene {b}: {name} of shape {a.shape} for {int(counts[b])} vehicles")
            parts.append(np.broadcast_to(a.reshape(-1) if a.ndim else a, (int(counts[b]),)))
        return np.concatenate(parts) if parts else np.zeros(0)
    a = np.asarray(v)
    if isinstance(v, np.ndarray) and a.ndim == 1 and a.shape[0] == M and a.dtype.kind in kinds:
        return a
    return np.repeat(_args.per_scene(v, name, B, kinds, shape_first=True), counts)


def pack_settings(item_off, max_turn=None, loop=False, ignore_walkers=False, **settings):
    """Settings -> (settings float32 (M, 13), flags uint8 (M,)) as sfm_batch_set_vehicle_autopilot takes them.  Each of ``SETTINGS``
    (default: ``DEFAULTS``), ``max_turn``, ``loop`` and ``ignore_walkers`` is one value, B values (per scene), a list of B entries
    (each one value or (M_b,) values) or an ndarray (M,) over all vehicles.  ``max_turn`` is the largest turn per tick as an angle
    in [0, pi/2): its cos and sin are taken in float64 and rounded once.  Raises ValueError on what the library would refuse."""
    io = np.asarray(item_off)
    M = int(io[-1])
    unknown = set(settings) - set(SETTINGS)
    if unknown:
        raise ValueError(f"unknown autopilot settings {sorted(unknown)}; known: {SETTINGS + ('max_turn', 'loop', 'ignore_walkers')}")
    out = np.zeros((M, N_SETTINGS), np.float32)
    for i, name in enumerate(SETTINGS):
        with np.errstate(over="ignore"):
            col = np.asarray(_per_vehicle(settings.get(name, DEFAULTS[name]), name, io), dtype=np.float64).astype(np.float32)
        if not (np.isfinite(col).all() and ((col > 0).all() if name in _STRICT else (col >= 0).all())):
            raise ValueError(f"{name} must be finite and {'> 0' if name in _STRICT else '>= 0'} in float32")
        out[:, i] = col
    if (out[:, 5] < out[:, 4]).any():
        raise ValueError("brake must be >= dec")
    with np.errstate(over="ignore"):
        if not np.isfinite((out[:, 9].astype(np.float64) ** 2).astype(np.float32)).all():
            raise ValueError("reach^2 must be finite in float32")
    turn = np.asarray(_per_vehicle(DEFAULTS["max_turn"] if max_turn is None else max_turn, "max_turn", io), dtype=np.float64)
    if not (np.isfinite(turn).all() and (turn >= 0).all() and (turn < np.pi / 2).all()):
        raise ValueError("max_turn must be an angle in [0, pi/2)")
    out[:, 11] = np.cos(turn).astype(np.float32)
    out[:, 12] = np.sin(turn).astype(np.float32)
    if M and not (out[:, 11] > 0).all():
        raise ValueError("max_turn: its cosine must be > 0 in float32")
    flags = np.zeros(M, np.uint8)
    for bit, (v, name) in ((FLAG_LOOP, (loop, "loop")), (FLAG_IGNORE_WALKERS, (ignore_walkers, "ignore_walkers"))):
        f = np.asarray(_per_vehicle(v, name, io, kinds="biu"))
        if M and not np.isin(f, (0, 1)).all():
            raise ValueError(f"{name} must hold booleans")
        flags |= (f.astype(np.uint8) * np.uint8(bit)).astype(np.uint8)
    return np.ascontiguousarray(out), flags


def _mx(x, y):
    return x if x > y else y


def idm_speed(s, u, gap, led, st, dt):
    """Step 5 of the rule in fp32, operation by operation: the speed along the heading ``s`` (already max(., 0)), the leader's speed
    along the heading ``u``, the ``gap`` to it (``led`` False: no leader), one row of settings and the step -> (a, s') float32."""
    f = np.float32
    s, u, gap, dt = f(s), f(u), f(gap), f(dt)
    v0, T, s0, acc, dec, brake = (f(x) for x in st[:6])
    with np.errstate(all="ignore"):
        q = s / v0
        q2 = q * q
        r4 = q2 * q2
        inter = f(0.0)
        if led:
            g = _mx(gap, GAP_FLOOR)
            dv = s - u
            k2 = f(2.0) * np.sqrt(acc * dec)
            dyn = f(_fma32(s, T, (s * dv) / k2))
            sstar = s0 + _mx(dyn, f(0.0))
            ratio = sstar / g
            inter = ratio * ratio
        araw = acc * ((f(1.0) - r4) - inter)
        a = _mx(araw, -brake)
        s1 = _mx(f(_fma32(dt, a, s)), f(0.0))
    return f(a), f(s1)


def idm_f64(s, u, gap, led, st, dt):
    """The float64 restatement of the speed rule (steps 4 and 5 behind the leader's choice), from the same fp32 inputs: the
    Intelligent Driver Model a = acc (1 - (s / v0)^4 - (s* / g)^2), s* = s0 + max(0, s T + s (s - u) / (2 sqrt(acc dec))), the gap
    floored at GAP_FLOOR, a >= -brake, s' = max(s + dt a, 0).  Returns (a, s') float64."""
    s, u, gap, dt = (np.float64(np.float32(x)) for x in (s, u, gap, dt))
    v0, T, s0, acc, dec, brake = (np.float64(np.float32(x)) for x in st[:6])
    inter = 0.0
    if led:
        g = max(gap, np.float64(GAP_FLOOR))
        sstar = s0 + max(s * T + s * (s - u) / (2.0 * np.sqrt(acc * dec)), 0.0)
        inter = (sstar / g) ** 2
    a = max(acc * (1.0 - (s / v0) ** 4 - inter), -brake)
    return a, max(s + dt * a, 0.0)


def equilibrium_gap(s, st):
    """The IDM's equilibrium gap behind a leader of the same speed ``s`` < v0, float64: (s0 + s T) / sqrt(1 - (s / v0)^4)."""
    v0, T, s0 = (np.float64(np.float32(x)) for x in st[:3])
    return (s0 + s * T) / np.sqrt(1.0 - (s / v0) ** 4)


def autopilot_vehicle(k, centres, velocities, headings, rings, peds, path, st, flags, cursor, dt):
    """One controller launch for vehicle ``k`` of one scene: ``centres``, ``velocities``, ``headings`` (M, 2) and ``rings`` (a list
    of (P_v, 2)) as the tick reads them, ``peds`` (N, 4) {x, y, vx, vy}, the vehicle's ``path`` (P, 2) with P >= 1, one row of
    settings ``st`` (13,), its ``flags``, its ``cursor`` and the scene's step ``dt`` -- all taken as fp32.  Returns
    (command (4,) float32, cursor int, record (8,) float32), bit for bit the kernel's."""
    f = np.float32
    ctr = np.asarray(centres, dtype=np.float64).astype(f).reshape(-1, 2)
    vel = np.asarray(velocities, dtype=np.float64).astype(f).reshape(-1, 2)
    head = np.asarray(headings, dtype=f).reshape(-1, 2)
    pk = np.asarray(peds, dtype=np.float64).astype(f).reshape(-1, 4)
    path = np.asarray(path, dtype=np.float64).astype(f).reshape(-1, 2)
    st = np.asarray(st, dtype=f).reshape(N_SETTINGS)
    P = len(path)
    cx, cy = ctr[k]
    hx, hy = head[k]
    rec = np.zeros(8, f)
    if not (abs(cx) < NEAR_LIMIT and abs(cy) < NEAR_LIMIT):            # 1. absent
        return STOP.copy(), int(cursor), rec
    v0, T, s0, acc, dec, brake, hw, front, look, reach, pm, cmax, smax = st
    reach2 = f(np.float64(reach) * np.float64(reach))
    loop = bool(int(flags) & FLAG_LOOP)
    with np.errstate(all="ignore"):
        def to(q):
            tx, ty = q[0] - cx, q[1] - cy
            return tx, ty, f(_fma32(tx, tx, ty * ty))
        cur = int(cursor)                                              # 2. the cursor
        tx, ty, n2 = to(path[cur])
        for _ in range(P):
            if not n2 < reach2:
                break
            if not loop and cur == P - 1:
                rec[0], rec[7] = cur, 1.0
                return STOP.copy(), cur, rec
            cur = 0 if cur + 1 == P else cur + 1
            tx, ty, n2 = to(path[cur])
        gx, gy = hx, hy                                                # 3. the turn
        if n2 > 0:
            nn = np.sqrt(n2)
            gx, gy = tx / nn, ty / nn
        cphi = f(_fma32(gx, hx, gy * hy))
        sphi = f(_fma32(gy, hx, -(gx * hy)))
        if cphi < cmax:
            cphi, sphi = cmax, (-smax if sphi < 0 else smax)
        best = None                                                    # 4. the leader: the minimum of (gap, kind, index)
        reachx = front + look

        def frame(x, y):
            rx, ry = x - cx, y - cy
            return _fma32(rx, hx, ry * hy), _fma32(rx, hy, -(ry * hx))
        if not int(flags) & FLAG_IGNORE_WALKERS and len(pk):
            al, ac = frame(pk[:, 0], pk[:, 1])
            live = (np.abs(pk[:, 0]) < NEAR_LIMIT) & (np.abs(pk[:, 1]) < NEAR_LIMIT)
            cand = live & (al > 0) & (np.abs(ac) < hw + pm) & (al < reachx)
            gap = (al - front) - pm
            if cand.any():
                j = int(np.flatnonzero(cand)[np.argmin(gap[cand])])    # (the first minimum: the lowest row)
                best = (gap[j], KIND_PEDESTRIAN, j, f(_fma32(pk[j, 2], hx, pk[j, 3] * hy)))
        for v in range(len(ctr)):
            if v == k or not (abs(ctr[v, 0]) < NEAR_LIMIT and abs(ctr[v, 1]) < NEAR_LIMIT):
                continue
            ring = np.asarray(rings[v], dtype=np.float64).astype(f).reshape(-1, 2)
            if not len(ring):
                continue
            al, ac = frame(ring[:, 0], ring[:, 1])
            cand = (al > 0) & (np.abs(ac) < hw) & (al < reachx)
            if cand.any():
                gap = f(np.min((al - front)[cand]))
                if best is None or (gap, KIND_VEHICLE, v) < best[:3]:
                    best = (gap, KIND_VEHICLE, v, f(_fma32(vel[v, 0], hx, vel[v, 1] * hy)))
        if not loop and cur == P - 1:
            gap = np.sqrt(n2)
            if best is None or (gap, KIND_PATH_END, 0) < best[:3]:
                best = (gap, KIND_PATH_END, 0, f(0.0))
        sp = f(_fma32(vel[k, 0], hx, vel[k, 1] * hy))                  # 5. the speed
        s = _mx(sp, f(0.0))
        a, s1 = idm_speed(s, best[3] if best else 0.0, best[0] if best else 0.0, best is not None, st, dt)
    if best is not None:
        rec[1:5] = best[1], best[2], best[0], best[3]
    rec[0], rec[5], rec[6] = cur, a, s1
    return np.array([s1, cphi, sphi, 2.0], f), cur, rec


def scene_vehicles(sc):
    """(centres (M,2) float32, velocities (M,2) float32, headings (M,2) float32, rings) of a scene dict or Scenario as the device
    holds them (``scenarios.vehicle_headings`` for the headings)."""
    from . import scenarios
    get, _ = scenarios._accessors(sc)
    dyn = list(get("dynamic_obstacles") or [])
    M = len(dyn)
    ctr = np.array([c for c, _ in dyn], dtype=np.float64).reshape(M, 2).astype(np.float32)
    vel = get("dynamic_vel")
    vel = np.zeros((M, 2), np.float32) if vel is None else np.asarray(vel, dtype=np.float64).reshape(M, 2).astype(np.float32)
    return ctr, vel, scenarios.vehicle_headings(sc), [np.asarray(r, dtype=np.float64).astype(np.float32) for _, r in dyn]


def autopilot_scene(sc, peds, paths, settings, flags, cursors, dt, commands=None):
    """The twin of one controller launch for ONE scene (a scene dict or Scenario with its vehicles as the next tick reads them):
    ``peds`` (N, 4) {x, y, vx, vy} (None: the scene's ``loc`` / ``vel``), ``paths`` one entry per vehicle (None or empty: not
    autopiloted), ``settings`` (M, 13) and ``flags`` (M,) as ``pack_settings`` returns them for the scene's vehicles, ``cursors``
    (M,), ``commands`` (M, 4) the command buffer before the launch (None: zeros).  Returns (commands (M, 4) float32, cursors (M,)
    int32, records (M, 8) float32); entries of vehicles that are not autopiloted come back as they went in (records: as zeros).
    Move the scene with ``scenarios.drive_vehicles(sc, commands[:, 3], commands[:, :3], dt)``."""
    from . import scenarios
    ctr, vel, head, rings = scene_vehicles(sc)
    M = len(ctr)
    if peds is None:
        get, _ = scenarios._accessors(sc)
        loc, v = np.asarray(get("loc"), dtype=np.float64), np.asarray(get("vel"), dtype=np.float64)
        peds = np.column_stack((loc[:, :2], v[:, :2])) if len(loc) else np.zeros((0, 4))
    cmds = np.zeros((M, 4), np.float32) if commands is None else np.array(commands, dtype=np.float32).reshape(M, 4)
    cur = np.array(cursors, dtype=np.int32).reshape(M)
    rec = np.zeros((M, 8), np.float32)
    st = np.asarray(settings, dtype=np.float32).reshape(M, N_SETTINGS)
    fl = np.asarray(flags).reshape(M)
    for k in range(M):
        p = None if paths[k] is None else np.asarray(paths[k], dtype=np.float64).reshape(-1, 2)
        if p is None or len(p) == 0:
            continue
        cmds[k], cur[k], rec[k] = autopilot_vehicle(k, ctr, vel, head, rings, peds, p, st[k], fl[k], cur[k], dt)
    return cmds, cur, rec
