"""The host twin of the batch's restart noise (sfm_batch_set_restart_noise; the rule: include/sfm_hip.h).

``resample_scene`` computes, in NumPy, what one noisy restart of one scene leaves on the device -- bit for bit: every random word is
the kernel's counter-based word (``reset_word``, the formula of sfm_device.h:
``h = mix32(seed ^ mix32(mix32(0x5BD1E995 ^ (8 i + c)) + 0x9E3779B9 (32 e + t)))``), every offset ``fmaf(2 u, ext, -ext)``
(``scan._fma32``), every distance ``fmaf(dx, dx, dy * dy)`` on fp32 differences (``observe._d2``) and every decision a strict ``<``
between fp32 values.  The rule rejects a proposal against the proposals of all lower-index rows of its round, accepted or not, so
the outcome is a function of the proposals alone and needs no order of evaluation.

Pure NumPy, no GPU and no library needed: a test, a host-driven reset or a data pipeline can state what the device samples.
"""
from __future__ import annotations

import numpy as np

from . import scenarios
from .observe import _d2, _f32, _get, _polylines, range2, live as _live
from .scan import _fma32

RESET_SALT = np.uint32(0x5BD1E995)
GOLDEN = np.uint32(0x9E3779B9)
MAX_TRIES = 32                       # SFM_BATCH_MAX_RESTART_TRIES
C_POS_X, C_POS_Y, C_GOAL_X, C_GOAL_Y, C_DELAY = range(5)     # the components of a random word
NOT_MOVABLE, FALLBACK = -2, -1       # ``detail["round"]`` of a row that is not movable / that no try could place


def mix32(a):
    """lowbias32 (sfm_device.h) on uint32 arrays."""
    a = np.array(a, dtype=np.uint32, copy=True)
    with np.errstate(over="ignore"):
        a ^= a >> np.uint32(16)
        a *= np.uint32(0x7FEB352D)
        a ^= a >> np.uint32(15)
        a *= np.uint32(0x846CA68B)
        a ^= a >> np.uint32(16)
    return a


def reset_word(seed, i, e, t, c):
    """The random word of component ``c`` of try ``t`` of restart ``e`` for item ``i`` (a row's index inside its scene, or a
    vehicle's) under ``seed``: uint32, all arithmetic modulo 2^32."""
    u32 = lambda v: np.asarray(v, dtype=np.uint64).astype(np.uint32)
    seed, i, e, t, c = (u32(v) for v in (seed, i, e, t, c))
    with np.errstate(over="ignore"):
        inner = mix32(RESET_SALT ^ (np.uint32(8) * i + c))
        return mix32(seed ^ mix32(inner + GOLDEN * (np.uint32(32) * e + t)))


def unit(h):
    """u = (h >> 8) * 2^-24 in [0, 1), float32 (exact)."""
    return ((np.asarray(h, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def offset(h, ext):
    """o = fmaf(2 u, ext, -ext) in [-ext, ext), float32; 2 u is exact."""
    ext = np.asarray(ext, dtype=np.float32)
    return _fma32(np.float32(2.0) * unit(h), ext, -ext)


def delay_ticks(h, D):
    """(uint64(h) * (D + 1)) >> 32: 0 .. D."""
    return int((int(h) * (int(D) + 1)) >> 32)


def _boxes(box, n, name):
    a = np.zeros((n, 2)) if box is None else np.asarray(box, dtype=np.float64)
    if a.ndim == 1 and a.shape[0] == 2:
        a = np.broadcast_to(a, (n, 2))
    if a.shape != (n, 2):
        raise ValueError(f"{name} of shape {a.shape} for {n} rows")
    return _f32(a, 2)


def resample_scene(scene, seed, episode, pos_box, goal_box=None, min_gap=0.0, point_gap=0.0, tries=8, state=None, vehicles=None,
                   waypoints=None, tracks=None, track_delay=None, tau=0, detail=False):
    """One noisy restart of one scene: (loc_xy (N,2) float32, waypoint_xy (N,2) float32, first_ticks (M,) int64, vehicles,
    fallbacks) -- what ``SfmBatch.state()``, ``waypoints()`` and ``dynamic_obstacles()`` return for the scene after the restart, its
    tracked vehicles' first ticks, and the scene's entry of ``restart_noise()[1]``.

    ``scene``: a scene dict as ``SfmBatch.upload`` takes it (or a ``scenarios.Scenario``).  ``seed``: the scene's seed; ``episode``:
    e, the scene's ``resets`` before this restart.  ``pos_box`` / ``goal_box``: (N,2) half-extents (one (2,) pair stands for every
    row; ``goal_box=None``: the goals stay).  ``min_gap`` / ``point_gap``: metres.  ``tries``: 1 .. 32.  The RESTORED state is fed
    in as for ``observe.observe_scene``: ``state`` = (loc, vel) as the snapshot holds them, ``vehicles`` = the scene's list of
    (center, ring) as restored, ``waypoints`` (N,2|3).  Traffic timing: ``tracks`` = one entry per vehicle, None or a track dict as
    ``batch.pack_tracks`` takes it whose ``first_tick`` is the RESTORED first tick (the snapshot's, moved by the ticks since);
    ``track_delay`` (M,) ints >= 0 or None; ``tau``: the batch's tick counter (``vehicle_tracks()[0]``).  The scene needs
    ``dynamic_yaw`` and ``dynamic_extent`` then (``scenarios.place_tracked`` places the vehicle again).

    ``detail=True`` appends a dict: ``round`` (N,) the round each row was placed in (NOT_MOVABLE, FALLBACK), and ``rejected``, the
    number of (row, round) rejections under each condition: ``blocker``, ``lower`` (a lower-index proposal of the same round),
    ``point``."""
    tries = int(tries)
    if not 1 <= tries <= MAX_TRIES:
        raise ValueError(f"tries must be 1 .. {MAX_TRIES}, got {tries}")
    seed, e = int(seed) & 0xFFFFFFFF, int(episode) & 0xFFFFFFFF
    loc = np.asarray(_get(scene, "loc") if state is None else state[0], dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    loc = loc.reshape(n, -1)
    x, y = (_f32(loc[:, 0], 0), _f32(loc[:, 1], 0)) if n else (np.zeros(0, np.float32), np.zeros(0, np.float32))
    wp = np.asarray(_get(scene, "waypoint") if waypoints is None else waypoints, dtype=np.float64).reshape(n, -1)
    wxy = _f32(wp[:, :2], 2) if n else np.zeros((0, 2), np.float32)
    gap2, pgap2 = range2(min_gap), range2(point_gap)
    idx = np.arange(n, dtype=np.uint32)

    # 5. traffic timing, before the rounds
    veh = list((_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles)
    M = len(veh)
    tracks = [None] * M if tracks is None else list(tracks)
    if len(tracks) != M:
        raise ValueError(f"{len(tracks)} tracks for {M} vehicles")
    first = np.array([0 if tr is None else int(tr["first_tick"]) for tr in tracks], dtype=np.int64)
    if track_delay is not None:
        D = np.asarray(track_delay).reshape(-1)
        if D.shape[0] != M or (D < 0).any():
            raise ValueError(f"track_delay must hold {M} values >= 0")
        moved = [k for k in range(M) if tracks[k] is not None and int(D[k]) > 0]
        if moved:
            for k in moved:
                first[k] += delay_ticks(reset_word(seed, k, e, 0, C_DELAY), D[k])
            sc = {"dynamic_obstacles": veh, "dynamic_vel": _get(scene, "dynamic_vel"), "dynamic_yaw": _get(scene, "dynamic_yaw"),
                  "dynamic_extent": _get(scene, "dynamic_extent")}
            again = scenarios.place_tracked(sc, [None if k not in moved else dict(tracks[k], first_tick=int(first[k])) for k in range(M)],
                                            tau)["dynamic_obstacles"]
            veh = [again[k] if k in moved else veh[k] for k in range(M)]
    points = np.concatenate([_polylines(_get(scene, "borders") or [], False)[0], _polylines(_get(scene, "static_obstacles") or [], True)[0],
                             _polylines(veh, True)[0]], axis=0)

    # 2. row classes
    hb = _boxes(pos_box, n, "pos_box")
    alive = _live(x, y)
    movable = alive & ~((hb[:, 0] == 0) & (hb[:, 1] == 0))
    blocker = alive & ~movable                                       # the fixed rows
    px, py = x.copy(), y.copy()                                       # final positions: blockers', and the snapshot's while a row is open
    opened = movable.copy()
    placed_in = np.full(n, NOT_MOVABLE, dtype=np.int64)
    placed_in[movable] = FALLBACK
    counts = {"blocker": 0, "lower": 0, "point": 0}

    # 3. placement rounds
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(tries):
            if not opened.any():
                break
            o = np.flatnonzero(opened)
            qx = x[o] + offset(reset_word(seed, idx[o], e, t, C_POS_X), hb[o, 0])
            qy = y[o] + offset(reset_word(seed, idx[o], e, t, C_POS_Y), hb[o, 1])
            bl = np.flatnonzero(blocker)
            r_block = (_d2(px[bl][None, :] - qx[:, None], py[bl][None, :] - qy[:, None]) < gap2).any(axis=1)
            lower = o[None, :] < o[:, None]
            r_lower = ((_d2(qx[None, :] - qx[:, None], qy[None, :] - qy[:, None]) < gap2) & lower).any(axis=1)
            r_point = np.zeros(o.shape[0], bool)
            if pgap2 > 0 and points.shape[0]:
                r_point = (_d2(qx[:, None] - points[None, :, 0], qy[:, None] - points[None, :, 1]) < pgap2).any(axis=1)
            for key, r in (("blocker", r_block), ("lower", r_lower), ("point", r_point)):
                counts[key] += int(r.sum())
            ok = o[~(r_block | r_lower | r_point)]
            px[ok], py[ok] = qx[~(r_block | r_lower | r_point)], qy[~(r_block | r_lower | r_point)]
            blocker[ok] = True
            opened[ok] = False
            placed_in[ok] = t

        # 6. goals
        if goal_box is not None and n:
            gb = _boxes(goal_box, n, "goal_box")
            a = np.flatnonzero(alive)
            wxy = wxy.copy()
            wxy[a, 0] = wxy[a, 0] + offset(reset_word(seed, idx[a], e, 0, C_GOAL_X), gb[a, 0])
            wxy[a, 1] = wxy[a, 1] + offset(reset_word(seed, idx[a], e, 0, C_GOAL_Y), gb[a, 1])

    out = (np.stack([px, py], axis=1), wxy, first, veh, int(opened.sum()))
    return out + ({"round": placed_in, "rejected": counts},) if detail else out


RESPAWN_SALT = np.uint32(0x2545F491)


def respawn_word(seed, i, e, t, c):
    """The random word of a row respawn: ``reset_word``'s formula under the constant 0x2545F491, with ``e`` the ROW's respawn counter
    (``row_resets[i]`` before the respawn) -- so a respawn's words never coincide with a scene restart's and never repeat."""
    u32 = lambda v: np.asarray(v, dtype=np.uint64).astype(np.uint32)
    seed, i, e, t, c = (u32(v) for v in (seed, i, e, t, c))
    with np.errstate(over="ignore"):
        inner = mix32(RESPAWN_SALT ^ (np.uint32(8) * i + c))
        return mix32(seed ^ mix32(inner + GOLDEN * (np.uint32(32) * e + t)))


def respawn_rows_scene(scene, chosen, snapshot_state, snapshot_waypoints, state, waypoints, row_resets=None, seed=None, pos_box=None,
                       goal_box=None, min_gap=0.0, point_gap=0.0, tries=8, vehicles=None, detail=False):
    """One respawn of the chosen rows of one scene (sfm_batch_respawn_rows_device): (loc (N,D) float32, vel (N,D) float32,
    waypoint_xy (N,2) float32, row_resets (N,) uint32, fallbacks) -- what ``SfmBatch.state()`` and ``waypoints()`` return for the
    scene after the respawn, the rows' respawn counters, and the scene's entry of ``row_respawns()[1]`` (None: no row is chosen, the
    device leaves the scene's counter alone).

    ``chosen``: (N,) nonzero = respawn the row.  ``snapshot_state`` = (loc, vel) and ``snapshot_waypoints`` (N,2|3): the rows as
    the snapshot holds them; ``state`` / ``waypoints``: as they are now.  ``seed=None``: restart noise is off -- the chosen rows are
    the snapshot's, the others stay (``row_resets`` comes back as given, ``fallbacks`` None).  With a seed the restart noise's
    rounds run for the chosen rows (``resample_scene``) with three changes: the words are ``respawn_word``'s with e = the row's
    ``row_resets`` (each chosen row's counter goes up by one); a chosen row is movable if it is live in the snapshot and has a
    nonzero ``pos_box``, and the blockers from the start are every live row that is not chosen where it stands NOW and every
    chosen live row with a zero box at its snapshot position; the points are ``scene``'s borders and static obstacles and
    ``vehicles`` (the scene's list of (center, ring) as they stand now; None: the scene's own).  ``detail=True`` appends the dict of
    ``resample_scene``."""
    sloc, svel = (np.asarray(a, dtype=np.float32) for a in snapshot_state)
    cloc, cvel = (np.asarray(a, dtype=np.float32) for a in state)
    n = cloc.shape[0] if cloc.ndim == 2 else 0
    ch = np.asarray(chosen).reshape(-1) != 0
    if ch.shape[0] != n:
        raise ValueError(f"{ch.shape[0]} choices for a scene of {n} pedestrians")
    swp = _f32(np.asarray(snapshot_waypoints, dtype=np.float64).reshape(n, -1)[:, :2], 2) if n else np.zeros((0, 2), np.float32)
    cwp = _f32(np.asarray(waypoints, dtype=np.float64).reshape(n, -1)[:, :2], 2) if n else np.zeros((0, 2), np.float32)
    loc, vel, wxy = cloc.copy(), cvel.copy(), cwp.copy()
    loc[ch], vel[ch], wxy[ch] = sloc[ch], svel[ch], swp[ch]
    resets = np.zeros(n, np.uint32) if row_resets is None else np.array(row_resets, dtype=np.uint32).reshape(n)
    info = {"round": np.full(n, NOT_MOVABLE, dtype=np.int64), "rejected": {"blocker": 0, "lower": 0, "point": 0}}
    if seed is None or not ch.any():
        out = (loc, vel, wxy, resets, None)
        return out + (info,) if detail else out
    tries = int(tries)
    if not 1 <= tries <= MAX_TRIES:
        raise ValueError(f"tries must be 1 .. {MAX_TRIES}, got {tries}")
    seed = int(seed) & 0xFFFFFFFF
    e = resets.copy()                                                 # read before this respawn
    resets[ch] += np.uint32(1)
    gap2, pgap2 = range2(min_gap), range2(point_gap)
    idx = np.arange(n, dtype=np.uint32)
    veh = list((_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles)
    points = np.concatenate([_polylines(_get(scene, "borders") or [], False)[0], _polylines(_get(scene, "static_obstacles") or [], True)[0],
                             _polylines(veh, True)[0]], axis=0)
    hb = _boxes(pos_box, n, "pos_box")
    x, y = loc[:, 0].copy(), loc[:, 1].copy()                         # after the copies: the snapshot's for chosen rows, the current for the rest
    alive = _live(x, y)
    movable = ch & alive & ~((hb[:, 0] == 0) & (hb[:, 1] == 0))
    blocker = alive & ~movable
    px, py = x.copy(), y.copy()
    opened = movable.copy()
    placed_in = info["round"]
    placed_in[movable] = FALLBACK
    counts = info["rejected"]
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(tries):
            if not opened.any():
                break
            o = np.flatnonzero(opened)
            qx = x[o] + offset(respawn_word(seed, idx[o], e[o], t, C_POS_X), hb[o, 0])
            qy = y[o] + offset(respawn_word(seed, idx[o], e[o], t, C_POS_Y), hb[o, 1])
            bl = np.flatnonzero(blocker)
            r_block = (_d2(px[bl][None, :] - qx[:, None], py[bl][None, :] - qy[:, None]) < gap2).any(axis=1)
            lower = o[None, :] < o[:, None]
            r_lower = ((_d2(qx[None, :] - qx[:, None], qy[None, :] - qy[:, None]) < gap2) & lower).any(axis=1)
            r_point = np.zeros(o.shape[0], bool)
            if pgap2 > 0 and points.shape[0]:
                r_point = (_d2(qx[:, None] - points[None, :, 0], qy[:, None] - points[None, :, 1]) < pgap2).any(axis=1)
            for key, r in (("blocker", r_block), ("lower", r_lower), ("point", r_point)):
                counts[key] += int(r.sum())
            good = ~(r_block | r_lower | r_point)
            ok = o[good]
            px[ok], py[ok] = qx[good], qy[good]
            blocker[ok] = True
            opened[ok] = False
            placed_in[ok] = t
        if goal_box is not None and n:
            gb = _boxes(goal_box, n, "goal_box")
            a = np.flatnonzero(ch & alive)
            wxy[a, 0] = wxy[a, 0] + offset(respawn_word(seed, idx[a], e[a], 0, C_GOAL_X), gb[a, 0])
            wxy[a, 1] = wxy[a, 1] + offset(respawn_word(seed, idx[a], e[a], 0, C_GOAL_Y), gb[a, 1])
    loc[:, 0], loc[:, 1] = px, py
    out = (loc, vel, wxy, resets, int(opened.sum()))
    return out + (info,) if detail else out
