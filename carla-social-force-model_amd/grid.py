"""The host twin of the batch's egocentric occupancy grids (sfm_batch_grid; the record and its rules: include/sfm_hip.h).

``grid_scene`` computes, in NumPy, the record ``SfmBatch.grids()`` returns for one scene -- bit for bit in BOTH frames: every
operation of the rules is one correctly rounded fp32 operation or an ``fmaf`` (``scan._fma32`` is an exact one), the heading of
frame 1 is ``scan.heading32``, and the velocity sums are formed by fp32 adds in ascending row order.  Per gridded live row a G x G
map centred on the row: how many other pedestrians stand in each cell, the sum of their velocities relative to the row, and how
many sampled points of borders, static-obstacle rings and vehicle rings lie in it.

``grid_vehicles_scene`` is the same for the vehicles' bird's-eye grid (sfm_batch_grid_vehicles, ``SfmBatch.vehicle_grids()``): a
GU x GV window around a point of the vehicle frame, turned by the stored heading, without the vehicle's own ring and with the other
vehicles' velocities per cell; ``vehicle_grid_arrays`` and ``vehicle_grid_slots`` pack its arguments.

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


def _slots(m, off):
    """(items int64 [M], counts int64 [B]): the items a bool mask ``m`` over them keeps (None: all), ascending, and how many of them
    lie between each pair of the ascending offsets ``off``."""
    items = np.arange(int(off[-1]), dtype=np.int64) if m is None else np.flatnonzero(m).astype(np.int64)
    return items, np.diff(np.searchsorted(items, off)).astype(np.int64)


def grid_slots(mask, scene_off):
    """Which rows are gridded -> (rows int64 [M], counts int64 [B]): the global row of every slot -- the slots are the masked rows
    of the whole batch in ascending order -- and how many slots each scene owns.  ``mask`` as ``scan.scan_mask`` takes it (None:
    every row).  Pure NumPy; raises ValueError."""
    so = np.asarray(scene_off, dtype=np.int64)
    if so.ndim != 1 or so.shape[0] < 1 or (np.diff(so) < 0).any():
        raise ValueError("scene_off must be B + 1 ascending offsets")
    return _slots(scan_mask(mask, so), so)


def _window_cells(fx, fy, c, GU, GV):
    """(inside, cell id cv * GU + cu) of sources at (fx, fy) in the window's frame: pu = fx / c + 0.5f GU, the division rounded
    first; pv likewise with GV."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        gu, gv = np.float32(GU), np.float32(GV)
        pu = ((fx / c).astype(np.float32) + np.float32(0.5) * gu).astype(np.float32)
        pv = ((fy / c).astype(np.float32) + np.float32(0.5) * gv).astype(np.float32)
        inside = (pu >= 0) & (pu < gu) & (pv >= 0) & (pv < gv)         # float compares: NaN and +-inf fail by themselves
    cu = np.where(inside, pu, np.float32(0)).astype(np.int32)          # (int)pu
    cv = np.where(inside, pv, np.float32(0)).astype(np.int32)
    return inside, cv * GU + cu


def _ordered_sums(cid, vx, vy, cells):
    """Per cell the count of the sources and the sums of (vx, vy) by fp32 adds from 0.0f in the order given: the q-th source of
    every cell is added in round q."""
    count = np.bincount(cid, minlength=cells).astype(np.float32)
    order = np.argsort(cid, kind="stable")
    sk = cid[order]
    rank = np.arange(len(sk)) - np.searchsorted(sk, sk, side="left")
    sx, sy = np.zeros(cells, np.float32), np.zeros(cells, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for q in range(int(rank.max()) + 1 if len(rank) else 0):
            pick = order[rank == q]
            sx[cid[pick]] = sx[cid[pick]] + vx[pick]
            sy[cid[pick]] = sy[cid[pick]] + vy[pick]
    return count, sx, sy


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
            inside, cid = _window_cells(fx, fy, c, G, G)
            # a source: a live row j != i; a gridded row that is not live reads zeros
            inside &= alive[None, :] & alive[i][:, None] & (np.arange(n)[None, :] != i[:, None])
            key = (slot * C2 + cid)[inside]                            # row-major: per gridded row, ascending j
            flat = rec[lo:lo + m]
            for ch, v in zip((CH_COUNT, CH_VX, CH_VY), _ordered_sums(key, rvx[inside], rvy[inside], m * C2)):
                flat[:, ch] = v.reshape(m, C2)
            for ch, pts in zip((CH_BORDER, CH_STATIC, CH_VEHICLE), geo):
                if len(pts) == 0:
                    continue
                fx, fy = rot(pts[None, :, 0] - xi, pts[None, :, 1] - yi)
                inside, cid = _window_cells(fx, fy, c, G, G)
                inside &= alive[i][:, None]
                flat[:, ch] = np.bincount((slot * C2 + cid)[inside], minlength=m * C2).reshape(m, C2)
    return rec.reshape(len(rows), GRID_CHANNELS, G, G)


# What follows is the vehicles' bird's-eye grid (sfm_batch_grid_vehicles), built from the same pieces.

MAX_VEHICLE_GRID_SIDE = 64           # SFM_BATCH_MAX_VEHICLE_GRID_SIDE: cells along one axis
MAX_VEHICLE_GRID_CELLS = 1024        # GU * GV
VEHICLE_GRID_CHANNELS = 8            # SFM_BATCH_VEHICLE_GRID_CHANNELS
VCH_COUNT, VCH_VX, VCH_VY, VCH_BORDER, VCH_STATIC, VCH_VEHICLE, VCH_VEHICLE_VX, VCH_VEHICLE_VY = range(8)


def check_window(GU, GV):
    """``GU``, ``GV`` -> ints, each 1 .. 64 cells and GU * GV <= 1024.  Raises ValueError."""
    for name, g in (("GU", GU), ("GV", GV)):
        if isinstance(g, (bool, np.bool_)) or not isinstance(g, (int, np.integer)) or not 1 <= int(g) <= MAX_VEHICLE_GRID_SIDE:
            raise ValueError(f"{name} must be an integer 1 .. {MAX_VEHICLE_GRID_SIDE} cells, got {g!r}")
    if int(GU) * int(GV) > MAX_VEHICLE_GRID_CELLS:
        raise ValueError(f"GU * GV must be at most {MAX_VEHICLE_GRID_CELLS} cells, got {int(GU) * int(GV)}")
    return int(GU), int(GV)


def check_centre(centre):
    """The middle of the window in the vehicle frame (x forward), metres -> (mx, my) float32; finite, |m| <= 1e6.  Raises
    ValueError."""
    from .scan import check_mount
    try:
        return check_mount(centre)
    except ValueError:
        raise ValueError("centre must be a pair (x, y) of numbers, finite and within 1e+06 metres of the vehicle's centre") from None


def _vehicle_mask(mask, item_off):
    """``mask`` -> bool [M] over the vehicles of all scenes in concatenated order, or None (every vehicle): a list / tuple with one
    entry per scene (None: every vehicle of the scene; one value; or M_b values), or one ndarray over the M vehicles."""
    io = np.asarray(item_off, dtype=np.int64)
    if io.ndim != 1 or io.shape[0] < 1 or (np.diff(io) < 0).any():
        raise ValueError("item_off must be B + 1 ascending offsets")
    B, M = len(io) - 1, int(io[-1])
    if mask is None:
        return None

    def rows(e, nb, where):
        a = np.asarray(e)
        if a.dtype.kind not in "biuf":
            raise ValueError(f"{where}mask must be booleans or numbers, got {a.dtype}")
        if a.ndim == 0:
            a = np.broadcast_to(a, (nb,))
        if a.size == 0 and nb == 0:
            a = np.zeros(0, bool)
        if a.shape != (nb,):
            raise ValueError(f"{where}mask of shape {a.shape} for {nb} vehicles")
        return a != 0

    if isinstance(mask, (list, tuple)):
        if len(mask) != B:
            raise ValueError(f"{len(mask)} entries of mask for {B} scenes (a list is per scene; pass an ndarray for all vehicles)")
        parts = [rows(True if e is None else e, int(io[b + 1] - io[b]), f"scene {b}: ") for b, e in enumerate(mask)]
        return np.concatenate(parts) if parts else np.zeros(0, bool)
    return rows(mask, M, "")


def vehicle_grid_arrays(item_off, GU, GV, cell, frame=0, mask=None, centre=(0.0, 0.0)):
    """Vehicle grid settings -> the arguments of sfm_batch_set_vehicle_grid: (GU, GV int, cell float32 [B], mask uint8 [M] or None,
    frame int, centre_x, centre_y float32).  ``item_off`` (B+1,): the vehicles' scene offsets.  ``cell`` as for ``grid_arrays``;
    ``mask``: None (every vehicle), a list with one entry per scene (None, one value or M_b values) or one array over the M
    vehicles; ``centre``: the middle of the window in the vehicle frame, metres, x forward.  Pure NumPy; raises ValueError on
    everything the library would refuse."""
    GU, GV = check_window(GU, GV)
    frame = check_frame(frame)
    m = _vehicle_mask(mask, item_off)
    c = per_scene_metres(cell, "cell", len(np.asarray(item_off)) - 1, True)
    mx, my = check_centre(centre)
    return GU, GV, c, None if m is None else np.ascontiguousarray(m, dtype=np.uint8), frame, mx, my


def vehicle_grid_slots(mask, item_off):
    """Which vehicles are gridded -> (vehicles int64 [M'], counts int64 [B]): the vehicle (in concatenated order) of every slot --
    the slots are the masked vehicles of the whole batch in ascending order -- and how many slots each scene owns.  ``mask`` as
    for ``vehicle_grid_arrays``.  Pure NumPy; raises ValueError."""
    return _slots(_vehicle_mask(mask, item_off), np.asarray(item_off, dtype=np.int64))


def grid_vehicles_scene(scene, GU, GV, cell, frame=0, mask=None, centre=(0.0, 0.0), state=None, vehicles=None, headings=None,
                        vehicle_vel=None):
    """The vehicle grid record of one scene, (m, 8, GV, GU) float32 with m the number of gridded vehicles (``mask``: bool (M_b,),
    None: all), as ``SfmBatch.vehicle_grids()`` returns it -- bit for bit in both frames (include/sfm_hip.h specifies the record).
    Channel 0 the number of live pedestrians per cell, 1 and 2 the sum of their velocities relative to the vehicle, 3 and 4 the
    number of border and static-obstacle points, 5 the number of ring points of the scene's OTHER vehicles, 6 and 7 the sum over
    those points of their owners' velocities relative to the vehicle.  Cell [cv][cu]: u along x (frame 1: forward).  A gridded
    vehicle that is not present reads zeros.

    ``scene``: a scene dict as ``SfmBatch.upload`` takes it (or a ``scenarios.Scenario``).  ``cell``: metres, this scene's.
    ``frame``: 0 world axes, 1 the vehicle's stored heading frame.  ``centre``: the middle of the window in the vehicle frame.
    What has changed on the device since the upload is fed in as for ``scan.scan_vehicles_scene``: ``state`` = (loc, vel) of the
    rows, ``vehicles`` = the scene's list of (center, ring), ``headings`` (M_b, 2) fp32 {cos, sin} (default:
    ``scenarios.vehicle_headings(scene)``), ``vehicle_vel`` (M_b, 2) (default: the scene's ``dynamic_vel``)."""
    from .scan import vehicle_scan_origin
    from .scenarios import vehicle_headings
    GU, GV = check_window(GU, GV)
    frame = check_frame(frame)
    c = per_scene_metres(cell, "cell", 1, True)[0]
    mx, my = check_centre(centre)
    veh = list((_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles)
    M = len(veh)
    if mask is None:
        gridded = np.ones(M, bool)
    else:
        gridded = np.asarray(mask)
        if gridded.shape != (M,):
            raise ValueError(f"a mask of shape {gridded.shape} for {M} vehicles")
        gridded = gridded != 0
    which = np.flatnonzero(gridded)
    cells = GU * GV
    rec = np.zeros((len(which), VEHICLE_GRID_CHANNELS, cells), np.float32)
    if len(which) == 0:
        return rec.reshape(len(which), VEHICLE_GRID_CHANNELS, GV, GU)
    h = _f32(vehicle_headings(scene) if headings is None else headings, 2)
    if h.shape != (M, 2):
        raise ValueError(f"headings of shape {h.shape} for {M} vehicles")
    vv = _get(scene, "dynamic_vel") if vehicle_vel is None else vehicle_vel
    vv = np.zeros((M, 2), np.float32) if vv is None else _f32(vv, 2)
    if vv.shape != (M, 2):
        raise ValueError(f"vehicle velocities of shape {vv.shape} for {M} vehicles")
    loc, vel = (_get(scene, "loc"), _get(scene, "vel")) if state is None else state
    loc, vel = np.asarray(loc, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    loc, vel = (loc.reshape(n, -1), vel.reshape(n, -1)) if n else (np.zeros((0, 3)),) * 2
    x, y, vx, vy = _f32(loc[:, 0], 0), _f32(loc[:, 1], 0), _f32(vel[:, 0], 0), _f32(vel[:, 1], 0)
    alive = _live(x, y)
    ctr = np.stack([_f32(ci, 0)[:2] for ci, _ in veh])
    rings = [_f32(r, 2) for _, r in veh]
    bpts = _polylines(_get(scene, "borders") or [], False)[0]
    spts = _polylines(_get(scene, "static_obstacles") or [], True)[0]
    present = _live(ctr[:, 0], ctr[:, 1])
    with np.errstate(over="ignore", invalid="ignore"):
        for slot, k in enumerate(which):
            if not present[k]:
                continue
            ox, oy = vehicle_scan_origin(ctr[k], h[k], (mx, my))
            rot = (lambda a, b: _rotate(h[k, 0], h[k, 1], a, b)) if frame == 1 else (lambda a, b: (a, b))
            r = rec[slot]
            # every live pedestrian, ascending j
            fx, fy = rot(x - ox, y - oy)
            inside, cid = _window_cells(fx, fy, c, GU, GV)
            inside &= alive
            rvx, rvy = rot(vx - vv[k, 0], vy - vv[k, 1])
            r[VCH_COUNT], r[VCH_VX], r[VCH_VY] = _ordered_sums(cid[inside], rvx[inside], rvy[inside], cells)
            for ch, pts in ((VCH_BORDER, bpts), (VCH_STATIC, spts)):
                if len(pts):
                    fx, fy = rot(pts[:, 0] - ox, pts[:, 1] - oy)
                    inside, cid = _window_cells(fx, fy, c, GU, GV)
                    r[ch] = np.bincount(cid[inside], minlength=cells)
            # the ring points of the other vehicles, ascending (vehicle, point), each with its owner's relative velocity
            others = [v for v in range(M) if v != k and len(rings[v])]
            if others:
                pts = np.concatenate([rings[v] for v in others], axis=0)
                owner = np.concatenate([np.full(len(rings[v]), v, np.int64) for v in others])
                fx, fy = rot(pts[:, 0] - ox, pts[:, 1] - oy)
                inside, cid = _window_cells(fx, fy, c, GU, GV)
                rvx, rvy = rot(vv[owner, 0] - vv[k, 0], vv[owner, 1] - vv[k, 1])
                r[VCH_VEHICLE], r[VCH_VEHICLE_VX], r[VCH_VEHICLE_VY] = _ordered_sums(cid[inside], rvx[inside], rvy[inside], cells)
    return rec.reshape(len(which), VEHICLE_GRID_CHANNELS, GV, GU)
