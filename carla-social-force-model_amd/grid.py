"""The host twin of the batch's egocentric occupancy grids (sfm_batch_grid; the record and its rules: include/sfm_hip.h).

``grid_scene`` computes, in NumPy, the record ``SfmBatch.grids()`` returns for one scene -- bit for bit in BOTH frames: every
operation of the rules is one correctly rounded fp32 operation or an ``fmaf`` (``scan._fma32`` is an exact one), the heading of
frame 1 is ``scan.heading32``, and the velocity sums are formed by fp32 adds in ascending row order.  Per gridded live row a G x G
map centred on the row: how many other pedestrians stand in each cell, the sum of their velocities relative to the row, and how
many sampled points of borders, static-obstacle rings and vehicle rings lie in it.

Pure NumPy, no GPU and no library needed.
"""
from __future__ import annotations

import numpy as np

from ._args import check_frame, per_scene_metres
from .observe import _f32, _get, _polylines, live as _live
from .scan import _fma32, heading32, scan_mask

MAX_GRID = 32                        # SFM_BATCH_MAX_GRID: cells per side
GRID_CHANNELS = 6                    # SFM_BATCH_GRID_CHANNELS
CH_COUNT, CH_VX, CH_VY, CH_BORDER, CH_STATIC, CH_VEHICLE = range(6)


def check_cells(G):
    """``G`` -> int, 1 .. 32 cells per side.  Raises ValueError."""
    if isinstance(G, (bool, np.bool_)) or not isinstance(G, (int, np.integer)) or not 1 <= int(G) <= MAX_GRID:
        raise ValueError(f"G must be an integer 1 .. {MAX_GRID} cells per side, got {G!r}")
    return int(G)


def grid_arrays(B, G, cell, frame=0):
    """Grid settings -> the arguments of sfm_batch_set_grid: (G int, cell float32 [B], frame int).  ``cell``: the cell size in
    metres, a scalar (broadcast to every scene) or B values, finite, > 0 and <= 1e6 in float32.  Pure NumPy; raises ValueError on a
    G outside 1 .. 32, a frame other than 0 or 1, a shape that does not fit, and every value the library would refuse."""
    B, G, frame = int(B), check_cells(G), check_frame(frame)
    return G, per_scene_metres(cell, "cell", B, True), frame


def grid_slots(mask, scene_off):
    """Which rows are gridded -> (rows int64 [M], counts int64 [B]): the global row of every slot -- the slots are the masked rows
    of the whole batch in ascending order -- and how many slots each scene owns.  ``mask`` as ``scan.scan_mask`` takes it (None:
    every row).  Pure NumPy; raises ValueError."""
    so = np.asarray(scene_off, dtype=np.int64)
    if so.ndim != 1 or so.shape[0] < 1 or (np.diff(so) < 0).any():
        raise ValueError("scene_off must be B + 1 ascending offsets")
    m = scan_mask(mask, so)
    rows = np.arange(int(so[-1]), dtype=np.int64) if m is None else np.flatnonzero(m).astype(np.int64)
    return rows, np.diff(np.searchsorted(rows, so)).astype(np.int64)


def _cells(fx, fy, c, half, G):
    """(inside, cell id) of sources at (fx, fy) in the grid's frame: pu = fx / c + half, the division rounded first."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        pu = ((fx / c).astype(np.float32) + half).astype(np.float32)
        pv = ((fy / c).astype(np.float32) + half).astype(np.float32)
        g = np.float32(G)
        inside = (pu >= 0) & (pu < g) & (pv >= 0) & (pv < g)           # float compares: NaN and +-inf fail by themselves
    cu = np.where(inside, pu, np.float32(0)).astype(np.int32)          # (int)pu
    cv = np.where(inside, pv, np.float32(0)).astype(np.int32)
    return inside, cv * G + cu


def _rotate(hx, hy, a, b):
    """(a, b) in the heading frame: (fmaf(hx, a, hy * b), fmaf(hx, b, -(hy * a)))."""
    with np.errstate(over="ignore", invalid="ignore"):
        return _fma32(hx, a, hy * b), _fma32(hx, b, -(hy * a))


def grid_scene(scene, G, cell, frame=0, mask=None, state=None, vehicles=None, waypoints=None):
    """The grid record of one scene, (m, 6, G, G) float32 with m the number of gridded rows (``mask``: bool (N,), None: all), as
    ``SfmBatch.grids()`` returns it: channel 0 the number of other live pedestrians per cell, 1 and 2 the sum of their relative
    velocities, 3, 4, 5 the number of border, static-obstacle and vehicle points.  Cell [cv][cu]: u along x (frame 1: forward).

    ``scene``: a scene dict as ``SfmBatch.upload`` takes it (or a ``scenarios.Scenario``).  ``cell``: metres, this scene's.
    ``frame``: 0 world axes, 1 heading frame.  What has changed on the device since the upload is fed in as for
    ``scan.scan_scene``: ``state`` = (loc, vel), ``vehicles`` = the scene's list of (center, ring), ``waypoints`` (N,2|3)."""
    G, c, frame = grid_arrays(1, G, cell, frame)
    c = c[0]
    half = np.float32(0.5) * np.float32(G)
    loc, vel = (_get(scene, "loc"), _get(scene, "vel")) if state is None else state
    loc, vel = np.asarray(loc, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    gridded = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool).reshape(n)
    rows = np.flatnonzero(gridded)
    rec = np.zeros((len(rows), GRID_CHANNELS, G * G), np.float32)
    if n == 0 or len(rows) == 0:
        return rec.reshape(len(rows), GRID_CHANNELS, G, G)
    loc, vel = loc.reshape(n, -1), vel.reshape(n, -1)
    x, y = _f32(loc[:, 0], 0), _f32(loc[:, 1], 0)
    vx, vy = _f32(vel[:, 0], 0), _f32(vel[:, 1], 0)
    alive = _live(x, y)
    if frame == 1:
        wp = np.asarray(_get(scene, "waypoint") if waypoints is None else waypoints, dtype=np.float64).reshape(n, -1)
        hx, hy = heading32(x, y, vx, vy, _f32(wp[:, 0], 0), _f32(wp[:, 1], 0))

    borders = _get(scene, "borders") or []
    statics = _get(scene, "static_obstacles") or []
    veh = (_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles
    geo = [_polylines(borders, False)[0], _polylines(statics, True)[0], _polylines(veh, True)[0]]

    C2 = G * G
    with np.errstate(over="ignore", invalid="ignore"):
        for lo in range(0, len(rows), 128):                            # chunked: the largest block is 128 x max(N, points)
            i = rows[lo:lo + 128]
            m = len(i)
            slot = np.arange(m)[:, None]                               # inside the chunk
            xi, yi = x[i][:, None], y[i][:, None]
            rot = (lambda a, b: _rotate(hx[i][:, None], hy[i][:, None], a, b)) if frame == 1 else (lambda a, b: (a, b))
            fx, fy = rot(x[None, :] - xi, y[None, :] - yi)
            rvx, rvy = rot(vx[None, :] - vx[i][:, None], vy[None, :] - vy[i][:, None])
            inside, cid = _cells(fx, fy, c, half, G)
            # a source: a live row j != i; a gridded row that is not live reads zeros
            inside &= alive[None, :] & alive[i][:, None] & (np.arange(n)[None, :] != i[:, None])
            key = (slot * C2 + cid)[inside]                            # row-major: per gridded row, ascending j
            rvx, rvy = rvx[inside], rvy[inside]
            flat = rec[lo:lo + m]
            flat[:, CH_COUNT] = np.bincount(key, minlength=m * C2).reshape(m, C2)
            # the sums: fp32 adds in ascending j from 0.0f -- the q-th source of every cell is added in round q
            order = np.argsort(key, kind="stable")
            sk = key[order]
            rank = np.arange(len(sk)) - np.searchsorted(sk, sk, side="left")
            sx, sy = np.zeros(m * C2, np.float32), np.zeros(m * C2, np.float32)
            for q in range(int(rank.max()) + 1 if len(rank) else 0):
                pick = order[rank == q]
                sx[key[pick]] = sx[key[pick]] + rvx[pick]
                sy[key[pick]] = sy[key[pick]] + rvy[pick]
            flat[:, CH_VX], flat[:, CH_VY] = sx.reshape(m, C2), sy.reshape(m, C2)
            for ch, pts in zip((CH_BORDER, CH_STATIC, CH_VEHICLE), geo):
                if len(pts) == 0:
                    continue
                fx, fy = rot(pts[None, :, 0] - xi, pts[None, :, 1] - yi)
                inside, cid = _cells(fx, fy, c, half, G)
                inside &= alive[i][:, None]
                flat[:, ch] = np.bincount((slot * C2 + cid)[inside], minlength=m * C2).reshape(m, C2)
    return rec.reshape(len(rows), GRID_CHANNELS, G, G)
