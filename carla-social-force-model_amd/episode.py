"""The host twin of the batch's episode ends (sfm_batch_end_step, ABI 16; the record and its rules: include/sfm_hip.h).

``episode_scene`` computes, in NumPy, the record row ``SfmBatch.episodes()`` returns for one scene and the scene's new episode state
-- bit for bit: every distance is formed as the kernel forms it, ``fmaf(dx, dx, dy * dy)`` on fp32 differences (``observe._d2``), a
minimum of floats without NaNs does not depend on the order it is taken in, and every decision is a strict ``<`` between fp32 values.

Pure NumPy, no GPU and no library needed: a test, a reward prototype or a host-driven loop can state what the device decides.
"""
from __future__ import annotations

import numpy as np

from .observe import _d2, _f32, _get, _polylines, range2, live as _live

EPISODE_WIDTH = 8
EP_DONE, EP_REASON, EP_AGE, EP_GOAL_D2, EP_PREV_GOAL_D2, EP_PED_D2, EP_VEH_D2, EP_WALL_D2 = range(8)
REASON_ARRIVED, REASON_TIME_LIMIT, REASON_PED_HIT, REASON_VEH_HIT, REASON_NOT_LIVE = 1, 2, 4, 8, 16
INF = np.float32(np.inf)


def radius2(radius):
    """r2 as the library forms it: the fp32 radius squared in double and rounded once (``observe.range2``)."""
    return range2(radius)


def _points_min(x, y, pts):
    """min over pts (P,2) fp32 of the tick's dist2(x, y, px, py); +inf without points.  fmin: a NaN operand is dropped, as fminf does."""
    if pts.shape[0] == 0:
        return INF
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(np.fmin.reduce(_d2(x - pts[:, 0], y - pts[:, 1]), initial=INF))


def episode_scene(scene, agent, radii, max_steps, age=0, prev=np.nan, state=None, vehicles=None, waypoints=None):
    """One evaluation of one scene: (record (8,) float32, (age, prev)) -- the row ``SfmBatch.episodes()`` returns for the scene after
    ``end_step()`` and the scene's episode state after it.

    ``scene``: a scene dict as ``SfmBatch.upload`` takes it (or a ``scenarios.Scenario``).  ``agent``: the agent's row, or -1.
    ``radii``: (goal_radius, ped_radius, veh_radius) in metres.  ``max_steps``: 0 = no time limit.  ``age`` / ``prev``: the episode
    state before the evaluation (0 and NaN after a restart).  What has changed on the device since the upload is fed in as for
    ``observe.observe_scene``: ``state`` = (loc, vel), ``vehicles`` = the scene's list of (center, ring), ``waypoints`` (N,2|3)."""
    agent, max_steps, age = int(agent), int(max_steps), int(age)
    rg2, rp2, rv2 = (radius2(r) for r in radii)
    loc = np.asarray(_get(scene, "loc") if state is None else state[0], dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    if agent != -1 and not 0 <= agent < n:
        raise ValueError(f"agent {agent} is no row of a scene of {n} pedestrians (-1: no agent)")
    prev = np.float32(prev)
    age += 1
    rec = np.full(EPISODE_WIDTH, INF, np.float32)
    reason = 0
    live = False
    if agent >= 0:
        loc = loc.reshape(n, -1)
        x, y = _f32(loc[:, 0], 0), _f32(loc[:, 1], 0)
        ok = _live(x, y)
        live = bool(ok[agent])
        if not live:
            reason = REASON_NOT_LIVE
    if live:
        xa, ya = x[agent], y[agent]
        wp = np.asarray(_get(scene, "waypoint") if waypoints is None else waypoints, dtype=np.float64).reshape(n, -1)
        wx, wy = _f32(wp[:, 0], 0), _f32(wp[:, 1], 0)
        with np.errstate(over="ignore", invalid="ignore"):
            goal_d2 = _d2(wx[agent:agent + 1] - xa, wy[agent:agent + 1] - ya)[0]
            others = ok.copy()
            others[agent] = False
            ped_d2 = np.float32(np.fmin.reduce(_d2(x[others] - xa, y[others] - ya), initial=INF)) if others.any() else INF
        veh = (_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles
        veh_d2 = _points_min(xa, ya, _polylines(veh, True)[0])
        wall_d2 = np.fmin(_points_min(xa, ya, _polylines(_get(scene, "borders") or [], False)[0]),
                          _points_min(xa, ya, _polylines(_get(scene, "static_obstacles") or [], True)[0]))
        rec[EP_GOAL_D2] = goal_d2
        rec[EP_PREV_GOAL_D2] = goal_d2 if np.isnan(prev) else prev
        rec[EP_PED_D2], rec[EP_VEH_D2], rec[EP_WALL_D2] = ped_d2, veh_d2, wall_d2
        prev = goal_d2
        reason = ((REASON_ARRIVED if goal_d2 < rg2 else 0) | (REASON_PED_HIT if ped_d2 < rp2 else 0) |
                  (REASON_VEH_HIT if veh_d2 < rv2 else 0))
    if max_steps > 0 and age >= max_steps:
        reason |= REASON_TIME_LIMIT
    rec[EP_DONE] = 1.0 if reason else 0.0
    rec[EP_REASON] = reason
    rec[EP_AGE] = age
    return rec, (age, prev)


def row_episode_scene(scene, agents, radii, max_steps, ages=None, prevs=None, state=None, vehicles=None, waypoints=None):
    """One evaluation of every agent ROW of one scene: (records (N,8) float32, done (N,) bool, ages (N,) int32, prevs (N,) float32)
    -- the scene's rows of ``SfmBatch.row_episodes()`` after ``end_row_step()``.

    ``agents``: (N,) nonzero = the row is an agent (or True / False for all).  ``radii`` / ``max_steps``: the scene's, as for
    ``episode_scene``.  ``ages`` / ``prevs``: the rows' episode state before the evaluation (None: zeros / NaN, as after a respawn).
    The rest as for ``episode_scene``.  The rules are ``episode_scene``'s with "the agent" read as "this agent row": ped_d2 is the
    minimum over all live rows j != i, other agents included.  Rows that are not agents keep what they are given: a zero record,
    done False and their state."""
    max_steps = int(max_steps)
    rg2, rp2, rv2 = (radius2(r) for r in radii)
    loc = np.asarray(_get(scene, "loc") if state is None else state[0], dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    ag = np.full(n, bool(agents)) if np.ndim(agents) == 0 else np.asarray(agents).reshape(-1) != 0
    if ag.shape[0] != n:
        raise ValueError(f"{ag.shape[0]} agent flags for a scene of {n} pedestrians")
    ages = np.zeros(n, np.int32) if ages is None else np.array(ages, dtype=np.int32).reshape(n)
    prevs = np.full(n, np.nan, np.float32) if prevs is None else np.array(prevs, dtype=np.float32).reshape(n)
    rec = np.zeros((n, EPISODE_WIDTH), np.float32)
    done = np.zeros(n, bool)
    if not ag.any():
        return rec, done, ages, prevs
    loc = loc.reshape(n, -1)
    x, y = _f32(loc[:, 0], 0), _f32(loc[:, 1], 0)
    ok = _live(x, y)
    wp = np.asarray(_get(scene, "waypoint") if waypoints is None else waypoints, dtype=np.float64).reshape(n, -1)
    wx, wy = _f32(wp[:, 0], 0), _f32(wp[:, 1], 0)
    veh = (_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles
    vpts = _polylines(veh, True)[0]
    bpts, spts = _polylines(_get(scene, "borders") or [], False)[0], _polylines(_get(scene, "static_obstacles") or [], True)[0]
    for i in np.flatnonzero(ag):
        age = int(ages[i]) + 1
        r = np.full(EPISODE_WIDTH, INF, np.float32)
        reason = REASON_NOT_LIVE
        if ok[i]:
            xa, ya = x[i], y[i]
            with np.errstate(over="ignore", invalid="ignore"):
                goal_d2 = _d2(wx[i:i + 1] - xa, wy[i:i + 1] - ya)[0]
                others = ok.copy()
                others[i] = False
                ped_d2 = np.float32(np.fmin.reduce(_d2(x[others] - xa, y[others] - ya), initial=INF)) if others.any() else INF
            veh_d2 = _points_min(xa, ya, vpts)
            wall_d2 = np.fmin(_points_min(xa, ya, bpts), _points_min(xa, ya, spts))
            r[EP_GOAL_D2] = goal_d2
            r[EP_PREV_GOAL_D2] = goal_d2 if np.isnan(prevs[i]) else prevs[i]
            r[EP_PED_D2], r[EP_VEH_D2], r[EP_WALL_D2] = ped_d2, veh_d2, wall_d2
            prevs[i] = goal_d2
            reason = ((REASON_ARRIVED if goal_d2 < rg2 else 0) | (REASON_PED_HIT if ped_d2 < rp2 else 0) |
                      (REASON_VEH_HIT if veh_d2 < rv2 else 0))
        if max_steps > 0 and age >= max_steps:
            reason |= REASON_TIME_LIMIT
        r[EP_DONE] = 1.0 if reason else 0.0
        r[EP_REASON] = reason
        r[EP_AGE] = age
        rec[i], done[i], ages[i] = r, bool(reason), age
    return rec, done, ages, prevs


REASON_WALL_HIT = 32             # SFM_EPISODE_WALL_HIT: set by vehicle records only
EP_PED_GAP2, EP_VEH_GAP2, EP_WALL_GAP2 = 5, 6, 7      # slots 5 .. 7 of a VEHICLE record


def box_gap2(centre, heading, extent, pts):
    """gap2 of include/sfm_hip.h for every point of ``pts`` (P,2) fp32: the squared distance to the box of half-extents ``extent``
    = (ex, ey) around ``centre``, turned by the stored ``heading`` = (cos, sin); 0 inside or on the box.  Bit for bit: the
    sensors' rotation in exact fused multiply-adds, every other operation one fp32 rounding.  A point that is not live gives +inf
    (it is no candidate), so the minimum over the result is the record's.  Returns float32 (P,)."""
    from .scan import _fma32
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    cx, cy = np.float32(centre[0]), np.float32(centre[1])
    hx, hy = np.float32(heading[0]), np.float32(heading[1])
    ex, ey = np.float32(extent[0]), np.float32(extent[1])
    out = np.full(pts.shape[0], INF, np.float32)
    ok = _live(pts[:, 0], pts[:, 1])
    if ok.any():
        with np.errstate(over="ignore", invalid="ignore"):
            dx, dy = pts[ok, 0] - cx, pts[ok, 1] - cy
            u = _fma32(hx, dx, hy * dy)
            v = _fma32(hx, dy, -(hy * dx))
            ax = np.fmax(np.abs(u) - ex, np.float32(0.0))
            ay = np.fmax(np.abs(v) - ey, np.float32(0.0))
            out[ok] = _fma32(ax, ax, ay * ay)
    return out


def _gap_min(centre, heading, extent, pts):
    return np.float32(np.fmin.reduce(box_gap2(centre, heading, extent, pts), initial=INF)) if len(pts) else INF


def vehicle_episode_scene(scene, agents, goals, extents, radii, max_steps, ages=None, prevs=None, state=None, vehicles=None, headings=None):
    """One evaluation of every agent VEHICLE of one scene: (records (M,8) float32, done (M,) bool, scene_done bool, ages (M,) int32,
    prevs (M,) float32) -- the scene's vehicles of ``SfmBatch.vehicle_episodes()`` after ``end_vehicle_step()``, and their episode
    state after it.

    ``agents``: (M,) nonzero = the vehicle is an agent (or True / False for all).  ``goals`` (M,2), ``extents`` (M,2) half-extents.
    ``radii``: (goal_radius, ped_radius, veh_radius, wall_radius) in metres; ``max_steps``: 0 = no time limit.  ``ages`` / ``prevs``:
    the vehicles' episode state before the evaluation (None: zeros / NaN, as after a respawn).  What has changed on the device since
    the upload is fed in: ``state`` = (loc, vel) of the rows, ``vehicles`` = the scene's list of (center, ring), ``headings`` (M,2)
    fp32 {cos, sin} (default: ``scenarios.vehicle_headings(scene)``).  Vehicles that are not agents keep what they are given: a zero
    record, done False and their state."""
    from .scan import _fma32
    from .scenarios import vehicle_headings
    max_steps = int(max_steps)
    rg2, rp2, rv2, rw2 = (radius2(r) for r in radii)
    veh = (_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles
    M = len(veh)
    ag = np.full(M, bool(agents)) if np.ndim(agents) == 0 else np.asarray(agents).reshape(-1) != 0
    if ag.shape[0] != M:
        raise ValueError(f"{ag.shape[0]} agent flags for a scene of {M} vehicles")
    ages = np.zeros(M, np.int32) if ages is None else np.array(ages, dtype=np.int32).reshape(M)
    prevs = np.full(M, np.nan, np.float32) if prevs is None else np.array(prevs, dtype=np.float32).reshape(M)
    rec = np.zeros((M, EPISODE_WIDTH), np.float32)
    done = np.zeros(M, bool)
    if not ag.any():
        return rec, done, False, ages, prevs
    loc = np.asarray(_get(scene, "loc") if state is None else state[0], dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    rows = _f32(loc.reshape(n, -1)[:, :2], 2) if n else np.zeros((0, 2), np.float32)
    g = _f32(goals, 2)
    ext = _f32(extents, 2)
    h = _f32(vehicle_headings(scene) if headings is None else headings, 2)
    ctr = np.stack([_f32(c, 0)[:2] for c, _ in veh])
    rings = [_f32(r, 2) for _, r in veh]
    wall = np.concatenate([_polylines(_get(scene, "borders") or [], False)[0], _polylines(_get(scene, "static_obstacles") or [], True)[0]])
    for k in np.flatnonzero(ag):
        age = int(ages[k]) + 1
        r = np.full(EPISODE_WIDTH, INF, np.float32)
        reason = REASON_NOT_LIVE
        if _live(ctr[k, 0], ctr[k, 1]):
            with np.errstate(over="ignore", invalid="ignore"):
                gx, gy = g[k, 0] - ctr[k, 0], g[k, 1] - ctr[k, 1]
                goal_d2 = np.float32(_fma32(gx, gx, gy * gy))
            others = [rings[q] for q in range(M) if q != k]
            other = np.concatenate(others) if others else np.zeros((0, 2), np.float32)
            ped, vg, wg = (_gap_min(ctr[k], h[k], ext[k], p) for p in (rows, other, wall))
            r[EP_GOAL_D2] = goal_d2
            r[EP_PREV_GOAL_D2] = goal_d2 if np.isnan(prevs[k]) else prevs[k]
            r[EP_PED_GAP2], r[EP_VEH_GAP2], r[EP_WALL_GAP2] = ped, vg, wg
            prevs[k] = goal_d2
            reason = ((REASON_ARRIVED if goal_d2 < rg2 else 0) | (REASON_PED_HIT if ped < rp2 else 0) |
                      (REASON_VEH_HIT if vg < rv2 else 0) | (REASON_WALL_HIT if wg < rw2 else 0))
        if max_steps > 0 and age >= max_steps:
            reason |= REASON_TIME_LIMIT
        r[EP_DONE] = 1.0 if reason else 0.0
        r[EP_REASON] = reason
        r[EP_AGE] = age
        rec[k], done[k], ages[k] = r, bool(reason), age
    return rec, done, bool(done.any()), ages, prevs
