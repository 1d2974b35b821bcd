"""The host twin of the batch's observations (sfm_batch_observe, ABI 15; the record and its rules: include/sfm_hip.h).

``observe_scene`` computes, in NumPy, the record ``SfmBatch.observations()`` returns for one scene -- bit for bit in frame 0, where
every value is one fp32 subtraction or a copy and every decision (who is a candidate, who comes first, which point is nearest, what
is in range) is taken on fp32 squared distances formed exactly as the kernel forms them: ``fmaf(dx, dx, dy * dy)``, written with the
idiom of ``scenarios.place_ring_f32`` (the product of two fp32 is exact in float64).  Frame 1 rotates that record into each row's
heading frame in float64 and rounds once; the kernel's fp32 rotation agrees with it to a few ulp.

Pure NumPy, no GPU and no library needed: a test, a reward prototype or a data pipeline can state what the device computes.
"""
from __future__ import annotations

import numpy as np

OBS_HEADER = 16
MAX_OBS_NEIGHBOURS = 16
NEAR_LIMIT = np.float32(1.0e12)      # sfm_device.h: a row is live while |x|, |y| < NEAR_LIMIT


def _get(scene, key, default=None):
    if isinstance(scene, dict):
        return scene.get(key, default)
    return getattr(scene, key, default)


def _f32(a, width):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(a.reshape(-1, width) if width else a.reshape(-1), dtype=np.float32)


def _d2(ax, ay):
    """fmaf(ax, ax, ay * ay) of fp32 arrays: ay * ay rounded to fp32, ax * ax exact in float64, one rounding of the sum."""
    with np.errstate(over="ignore", invalid="ignore"):
        yy = (ay * ay).astype(np.float64)
        xx = ax.astype(np.float64) * ax.astype(np.float64)
        return (xx + yy).astype(np.float32)


def live(x, y):
    """Which rows are live, as the three sensor kernels decide it (row_live, sfm_device.h); a NaN position fails it."""
    return (np.abs(x) < NEAR_LIMIT) & (np.abs(y) < NEAR_LIMIT)


def range2(sense_range):
    """R2 as the library forms it: the fp32 range squared in double and rounded once."""
    r = np.float64(np.float32(sense_range))
    return np.float32(r * r)


def _polylines(items, rings):
    """Concatenated fp32 points of one kind and, per point, the index of its polyline."""
    pts = [_f32(p, 2) for p in (items if not rings else [it[1] for it in items])]
    which = [np.full(len(p), q, dtype=np.int64) for q, p in enumerate(pts)]
    if not pts:
        return np.zeros((0, 2), np.float32), np.zeros(0, np.int64)
    return np.concatenate(pts, axis=0), np.concatenate(which)


def _nearest(x, y, pts, R2):
    """Per row: (present (N,) bool, index (N,) of the first minimum of d2 over pts).  Without points nobody sees one."""
    n = x.shape[0]
    if pts.shape[0] == 0:
        return np.zeros(n, bool), np.zeros(n, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        d2 = _d2(x[:, None] - pts[None, :, 0], y[:, None] - pts[None, :, 1])
    idx = np.argmin(d2, axis=1)                                        # the first minimum: polylines in order, points in order
    return d2[np.arange(n), idx] < R2, idx


def candidate_counts(scene, sense_range, state=None):
    """Per row, how many neighbour candidates it has (rows j != i of the scene with d2 < R2), before the cut to k slots: (N,) int64.
    Rows that are not live count too (their record is zero whatever they have)."""
    loc = np.asarray(_get(scene, "loc") if state is None else state[0], dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    if n == 0:
        return np.zeros(0, np.int64)
    loc = loc.reshape(n, -1)
    x, y = _f32(loc[:, 0], 0), _f32(loc[:, 1], 0)
    with np.errstate(over="ignore", invalid="ignore"):
        d2 = _d2(x[None, :] - x[:, None], y[None, :] - y[:, None])
    return ((d2 < range2(sense_range)) & ~np.eye(n, dtype=bool)).sum(axis=1)


def heading(rec0):
    """The heading (N,2) float64 of every row of a frame-0 record: v / |v| when fmaf(vx, vx, vy * vy) > 0, else the goal's direction
    when fmaf(gx, gx, gy * gy) > 0, else (1, 0).  The tests are on fp32 values, the division is in float64.
    ``scan.heading32`` is the same rule in the kernels' own fp32 arithmetic, for tests that compare bit for bit."""
    rec0 = np.asarray(rec0, dtype=np.float32)
    g, v = rec0[:, 0:2], rec0[:, 2:4]
    vv, gg = _d2(v[:, 0], v[:, 1]), _d2(g[:, 0], g[:, 1])
    h = np.zeros((rec0.shape[0], 2))
    h[:, 0] = 1.0
    use_v = vv > 0
    use_g = ~use_v & (gg > 0)
    for use, w in ((use_v, v), (use_g, g)):
        w64 = w[use].astype(np.float64)
        h[use] = w64 / np.sqrt(w64[:, 0] ** 2 + w64[:, 1] ** 2)[:, None]
    return h


def rotate_record(rec0, h):
    """Every 2-vector (a, b) of a frame-0 record -> (h_x a + h_y b, -h_y a + h_x b), in float64 (not rounded): the goal, the own
    velocity, both halves of the vehicle entry, the border and static entries, both halves of every slot.  Floats 4 .. 7 stay."""
    out = np.asarray(rec0, dtype=np.float64).copy()
    hx, hy = h[:, 0], h[:, 1]
    for c in [0, 2] + list(range(8, out.shape[1], 2)):
        a, b = out[:, c].copy(), out[:, c + 1].copy()
        out[:, c] = hx * a + hy * b
        out[:, c + 1] = -hy * a + hx * b
    return out


def observe_scene(scene, k, sense_range, frame=0, state=None, vehicles=None, vehicle_vel=None, waypoints=None, target_speed=None):
    """The observation record of one scene, (N, 16 + 4k) float32, as ``SfmBatch.observations()`` returns it.

    ``scene``: a scene dict as ``SfmBatch.upload`` takes it (or a ``scenarios.Scenario``).  ``k``: neighbour slots, 1 .. 16;
    ``sense_range``: metres; ``frame``: 0 world axes, 1 heading frame.  What has changed on the device since the upload is fed in:
    ``state`` = (loc (N,2|3), vel (N,2|3)) as ``SfmBatch.state()`` gives it for the scene; ``vehicles`` = the scene's list of
    (center, ring) as ``SfmBatch.dynamic_obstacles()`` gives it, with ``vehicle_vel`` (M,2) where the velocities changed too
    (default: the scene's ``dynamic_vel``, None at rest); ``waypoints`` (N,2|3) and ``target_speed`` (N,) likewise."""
    k = int(k)
    if not 1 <= k <= MAX_OBS_NEIGHBOURS:
        raise ValueError(f"k must be 1 .. {MAX_OBS_NEIGHBOURS}, got {k}")
    if frame not in (0, 1):
        raise ValueError(f"frame must be 0 or 1, got {frame!r}")
    R2 = range2(sense_range)
    loc, vel = (_get(scene, "loc"), _get(scene, "vel")) if state is None else state
    loc, vel = np.asarray(loc, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    W = OBS_HEADER + 4 * k
    rec = np.zeros((n, W), np.float32)
    if n == 0:
        return rec
    loc, vel = loc.reshape(n, -1), vel.reshape(n, -1)
    x, y = _f32(loc[:, 0], 0), _f32(loc[:, 1], 0)
    vx, vy = _f32(vel[:, 0], 0), _f32(vel[:, 1], 0)
    wp = np.asarray(_get(scene, "waypoint") if waypoints is None else waypoints, dtype=np.float64).reshape(n, -1)
    wx, wy = _f32(wp[:, 0], 0), _f32(wp[:, 1], 0)
    ts = _f32(_get(scene, "target_speed") if target_speed is None else target_speed, 0)

    with np.errstate(over="ignore", invalid="ignore"):
        # neighbours: the first k candidates in ascending (d2, j) order -- a stable sort of d2 over ascending j
        dx, dy = x[None, :] - x[:, None], y[None, :] - y[:, None]
        d2 = _d2(dx, dy)
        cand = (d2 < R2) & ~np.eye(n, dtype=bool)
        order = np.argsort(np.where(cand, d2, np.float32(np.inf)), axis=1, kind="stable")[:, :k]
        m = np.minimum(cand.sum(axis=1), k)
        rec[:, 0], rec[:, 1] = wx - x, wy - y
        rec[:, 2], rec[:, 3] = vx, vy
        rec[:, 4] = ts
        rec[:, 5] = 1.0
        rec[:, 6] = m
        for s in range(min(k, n)):
            j = order[:, s]
            filled = s < m
            for c, (col, own) in enumerate(((x, x), (y, y), (vx, vx), (vy, vy))):
                rec[:, OBS_HEADER + 4 * s + c] = np.where(filled, col[j] - own, np.float32(0.0))

        # nearest points per kind: borders, static obstacles, vehicles
        borders = _get(scene, "borders") or []
        statics = _get(scene, "static_obstacles") or []
        veh = (_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles
        vv = _get(scene, "dynamic_vel") if vehicle_vel is None else vehicle_vel
        vv = np.zeros((len(veh), 2), np.float32) if vv is None else _f32(vv, 2)
        flags = np.zeros(n, np.float32)
        for bit, col, (pts, which) in ((1, 12, _polylines(borders, False)), (2, 14, _polylines(statics, True)), (4, 8, _polylines(veh, True))):
            present, idx = _nearest(x, y, pts, R2)
            if not present.any():
                continue
            p = pts[idx]
            rec[:, col] = np.where(present, p[:, 0] - x, np.float32(0.0))
            rec[:, col + 1] = np.where(present, p[:, 1] - y, np.float32(0.0))
            if bit == 4:
                ov = vv[which[idx]]
                rec[:, 10] = np.where(present, ov[:, 0] - vx, np.float32(0.0))
                rec[:, 11] = np.where(present, ov[:, 1] - vy, np.float32(0.0))
            flags += np.where(present, np.float32(bit), np.float32(0.0))
        rec[:, 7] = flags
    rec[~live(x, y)] = 0.0
    if frame == 1:
        with np.errstate(over="ignore", invalid="ignore"):
            rec = rotate_record(rec, heading(rec)).astype(np.float32)
    return rec


def rotate_vehicle_record(rec0, h):
    """Frame 1 of a vehicle record from its frame-0 record and the stored headings ``h`` (M,2) float32, bit for bit: every 2-vector
    (p, q) except floats 4-5 becomes (fmaf(hx, p, hy * q), fmaf(hx, q, -(hy * p))) -- floats 0-1, 2-3, 10-11, 12-13 and both halves
    of every slot; floats 4 .. 9, 14 and 15 stay.  A pure function of the frame-0 record and ``h``."""
    from .scan import _fma32
    out = np.array(rec0, dtype=np.float32, copy=True)
    h = np.asarray(h, dtype=np.float32).reshape(-1, 2)
    hx, hy = h[:, 0], h[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        for c in [0, 2, 10, 12] + list(range(OBS_HEADER, out.shape[1], 2)):
            p, q = out[:, c].copy(), out[:, c + 1].copy()
            out[:, c] = _fma32(hx, p, hy * q)
            out[:, c + 1] = _fma32(hx, q, -(hy * p))
    out[rec0[:, 6] == 0] = 0.0                                         # (absent or masked out: the whole record is zeros)
    return out


def observe_vehicles_scene(scene, k, sense_range, frame=0, goals=None, mask=None, state=None, vehicles=None, vehicle_vel=None,
                           headings=None):
    """The vehicle observation record of one scene, (M, 16 + 4k) float32, as ``SfmBatch.vehicle_observations()`` returns it -- bit
    for bit in both frames (include/sfm_hip.h specifies the record; every decision is taken on fp32 squared distances formed as the
    kernel forms them, and frame 1's rotation is written in exact fused multiply-adds).

    ``scene``: a scene dict as ``SfmBatch.upload`` takes it (or a ``scenarios.Scenario``).  ``goals`` (M,2) or None (zeros);
    ``mask`` (M,) or None (every vehicle).  What has changed on the device since the upload is fed in: ``state`` = (loc, vel) of
    the rows, ``vehicles`` = the scene's list of (center, ring), ``vehicle_vel`` (M,2), ``headings`` (M,2) fp32 {cos, sin}
    (default: ``scenarios.vehicle_headings(scene)``)."""
    from .scan import _fma32
    from .scenarios import vehicle_headings
    k = int(k)
    if not 1 <= k <= MAX_OBS_NEIGHBOURS:
        raise ValueError(f"k must be 1 .. {MAX_OBS_NEIGHBOURS}, got {k}")
    if frame not in (0, 1):
        raise ValueError(f"frame must be 0 or 1, got {frame!r}")
    R2 = range2(sense_range)
    veh = (_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles
    M = len(veh)
    rec = np.zeros((M, OBS_HEADER + 4 * k), np.float32)
    if M == 0:
        return rec
    loc, vel = (_get(scene, "loc"), _get(scene, "vel")) if state is None else state
    loc, vel = np.asarray(loc, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    loc, vel = (loc.reshape(n, -1), vel.reshape(n, -1)) if n else (np.zeros((0, 3)),) * 2
    x, y = (_f32(loc[:, 0], 0), _f32(loc[:, 1], 0)) if n else (np.zeros(0, np.float32),) * 2
    vx, vy = (_f32(vel[:, 0], 0), _f32(vel[:, 1], 0)) if n else (np.zeros(0, np.float32),) * 2
    alive = live(x, y)
    vv = _get(scene, "dynamic_vel") if vehicle_vel is None else vehicle_vel
    vv = np.zeros((M, 2), np.float32) if vv is None else _f32(vv, 2)
    h = _f32(vehicle_headings(scene) if headings is None else headings, 2)
    g = np.zeros((M, 2), np.float32) if goals is None else _f32(goals, 2)
    mk = np.ones(M, bool) if mask is None else np.asarray(mask).reshape(M) != 0
    ctr = np.stack([_f32(c, 0) for c, _ in veh])
    bpts, _ = _polylines(_get(scene, "borders") or [], False)
    spts, _ = _polylines(_get(scene, "static_obstacles") or [], True)
    inf = np.float32(np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        present = live(ctr[:, 0], ctr[:, 1])
        for v in range(M):
            if not (mk[v] and present[v]):
                continue
            cx, cy = ctr[v]
            r = rec[v]
            r[0], r[1] = g[v, 0] - cx, g[v, 1] - cy
            r[2], r[3] = vv[v]
            r[4], r[5] = h[v]
            r[6] = 1.0
            # neighbours: the first k live rows with d2 < R2 in ascending (d2, j) order -- a stable sort over ascending j
            d2 = _d2(x - cx, y - cy)
            cand = alive & (d2 < R2)
            order = np.argsort(np.where(cand, d2, inf), kind="stable")[:k]
            m = min(int(cand.sum()), k)
            r[7] = m
            for s in range(m):
                j = order[s]
                r[OBS_HEADER + 4 * s:OBS_HEADER + 4 * s + 4] = (x[j] - cx, y[j] - cy, vx[j] - vv[v, 0], vy[j] - vv[v, 1])
            # clear_d2: ring points x live rows; a NaN distance is no candidate
            ring = _f32(veh[v][1], 2)
            clear = inf
            if ring.shape[0] and alive.any():
                dd = _d2(x[alive][:, None] - ring[None, :, 0], y[alive][:, None] - ring[None, :, 1])
                dd = dd[~np.isnan(dd)]
                clear = dd.min() if dd.size else inf
            r[8] = clear
            others = present & (np.arange(M) != v)
            od = _d2(ctr[others, 0] - cx, ctr[others, 1] - cy)
            od = od[~np.isnan(od)]
            r[9] = od.min() if od.size else inf
            flags = 0
            for bit, col, pts in ((1, 10, bpts), (2, 12, spts)):
                if pts.shape[0] == 0:
                    continue
                pd = _d2(pts[:, 0] - cx, pts[:, 1] - cy)
                pd = np.where(np.isnan(pd), inf, pd)
                i = int(np.argmin(pd))                                 # the first minimum: polylines in order, points in order
                if pd[i] < R2:
                    r[col], r[col + 1] = pts[i, 0] - cx, pts[i, 1] - cy
                    flags += bit
            r[14] = flags
            r[15] = _fma32(vv[v, 0], h[v, 0], vv[v, 1] * h[v, 1])
    if frame == 1:
        rec = rotate_vehicle_record(rec, h)
    return rec
