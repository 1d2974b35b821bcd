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
