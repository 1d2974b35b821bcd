"""The host twin of the batch's range scans (sfm_batch_scan, ABI 17; the record and its rules: include/sfm_hip.h).

``scan_scene`` computes, in NumPy, the record ``SfmBatch.scans()`` returns for one scene -- bit for bit in BOTH frames: every
operation of the rules is one correctly rounded fp32 operation or an ``fmaf``, and ``_fma32`` is an exact ``fmaf`` (the float64 sum
is repaired to round-to-odd before the cast, so it is never rounded twice).  Per scanned live row and ray: the distance to the first
disc the ray meets -- pedestrians are discs of ``ped_radius``, every sampled point of a border, a static-obstacle ring or a vehicle
ring is a disc of ``point_radius`` -- and the kind of what was hit.

Pure NumPy, no GPU and no library needed.
"""
from __future__ import annotations

import numpy as np

from ._args import MAX_METRES as MAX_SCAN_RANGE, check_frame, per_scene_metres
from .observe import _f32, _get, _polylines, live as _live

MAX_SCAN_RAYS = 64                   # SFM_BATCH_MAX_SCAN_RAYS
MAX_VEHICLE_SCAN_RAYS = 256          # SFM_BATCH_MAX_VEHICLE_SCAN_RAYS
KIND_NONE, KIND_PEDESTRIAN, KIND_BORDER, KIND_STATIC, KIND_VEHICLE = range(5)
POINT_RADIUS = 0.1                   # the reference's sampling resolution of borders and rings


def _fma32(a, b, c):
    """fmaf(a, b, c) of fp32 arrays, exact: the product of two fp32 is exact in float64; the float64 sum s = RN(p + c) can be off
    the true sum by a residual e (TwoSum gives it exactly), and casting s to fp32 would then round a second time.  Where e != 0
    the sum is moved to its odd neighbour on e's side (round-to-odd); a round-to-odd float64 cast to fp32 rounds as the exact sum
    does (53 >= 24 + 2 bits).  Returns float32."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p                                                     # TwoSum (Knuth): e = (p + c) - s exactly, for finite s
        e = (p - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & (e != 0)
        bits = np.array(s, dtype=np.float64, copy=True).view(np.int64)
        even = (bits & 1) == 0
        away = (e > 0) == (s > 0)                                      # the true sum lies further from zero than s
        bits = np.where(fix & even, bits + np.where(away, 1, -1), bits)
        return bits.view(np.float64).astype(np.float32)


def radius2(r):
    """r2 as the library forms it: the fp32 radius squared in double and rounded once (like ``observe.range2``)."""
    r = np.float64(np.float32(r))
    return np.float32(r * r)


def default_angles(R, limit=MAX_SCAN_RAYS):
    """The default ray angles: 2 pi q / R, q = 0 .. R-1, float64.  ``limit``: the most rays the sensor takes (64 for the rows' scan,
    ``MAX_VEHICLE_SCAN_RAYS`` for the vehicles')."""
    R = int(R)
    if not 1 <= R <= limit:
        raise ValueError(f"R must be 1 .. {limit} rays, got {R}")
    return 2.0 * np.pi * np.arange(R) / R


def ray_directions(angles, limit=MAX_SCAN_RAYS):
    """Ray angles (radians, 1 .. ``limit`` of them, 64 unless said otherwise) -> (dir_x, dir_y) float32 [R]: cos and sin formed in
    double and rounded once.  Pure NumPy; raises ValueError on a shape that does not fit and on an angle that is not finite."""
    a = np.asarray(angles)
    if a.dtype.kind not in "iuf":
        raise ValueError(f"angles must be numbers, got {a.dtype}")
    a = a.astype(np.float64)
    if a.ndim != 1 or not 1 <= a.shape[0] <= limit:
        raise ValueError(f"angles: expected 1 .. {limit} values, got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError("angles must be finite")
    return np.ascontiguousarray(np.cos(a), dtype=np.float32), np.ascontiguousarray(np.sin(a), dtype=np.float32)


def check_directions(directions, limit=MAX_SCAN_RAYS):
    """(dir_x, dir_y) given directly -> both as float32 [R], used as given (not renormalised).  Raises ValueError on shapes that do
    not fit, R outside 1 .. ``limit`` (64 unless said otherwise) and values that are not finite in float32."""
    try:
        dx, dy = directions
    except (TypeError, ValueError):
        raise ValueError("directions must be a pair (dir_x, dir_y)") from None
    dx, dy = np.asarray(dx), np.asarray(dy)
    if dx.dtype.kind not in "iuf" or dy.dtype.kind not in "iuf":
        raise ValueError("directions must be numbers")
    if dx.ndim != 1 or dx.shape != dy.shape or not 1 <= dx.shape[0] <= limit:
        raise ValueError(f"directions: expected two arrays of 1 .. {limit} values, got shapes {dx.shape} and {dy.shape}")
    with np.errstate(over="ignore"):
        dx, dy = np.ascontiguousarray(dx, dtype=np.float32), np.ascontiguousarray(dy, dtype=np.float32)
    if not (np.isfinite(dx).all() and np.isfinite(dy).all()):
        raise ValueError("directions must be finite in float32")
    return dx, dy


def scan_arrays(B, max_range, ped_radius, point_radius=POINT_RADIUS, frame=0):
    """Scan settings -> the per-scene arguments of sfm_batch_set_scan: (max_range, ped_radius, point_radius float32 [B], frame int).
    Each of the three is a scalar (broadcast to every scene, like ``stream_arrays``) or B values, in metres: ``max_range`` finite,
    > 0 and <= 1e6 in float32; the radii finite, >= 0 and <= 1e6 (0 switches the kind off).  Pure NumPy; raises ValueError on a
    frame other than 0 or 1, a shape that does not fit, and every value the library would refuse."""
    B, frame = int(B), check_frame(frame)
    return (per_scene_metres(max_range, "max_range", B, True), per_scene_metres(ped_radius, "ped_radius", B, False),
            per_scene_metres(point_radius, "point_radius", B, False), frame)


def scan_mask(mask, scene_off):
    """Which rows are scanned -> uint8 [N_total], or None for every row.  ``mask``: None; a list with one entry per scene (each a
    bool array (N_b,), one bool for the whole scene, or row indices inside the scene as integers); or one bool ndarray (N_total,)
    over the concatenated rows.  Pure NumPy; raises ValueError."""
    if mask is None:
        return None
    so = np.asarray(scene_off)
    B, n = len(so) - 1, int(so[-1])
    if isinstance(mask, (list, tuple)):
        if len(mask) != B:
            raise ValueError(f"{len(mask)} entries of mask for {B} scenes (a list is per scene; pass an ndarray for concatenated rows)")
        out = np.zeros(n, np.uint8)
        for b, e in enumerate(mask):
            nb = int(so[b + 1] - so[b])
            a = np.asarray(e)
            if a.dtype.kind == "b":
                if a.ndim == 0:
                    a = np.broadcast_to(a, (nb,))
                if a.shape != (nb,):
                    raise ValueError(f"scene {b}: a bool mask of shape {a.shape} for {nb} rows")
                out[so[b]:so[b + 1]] = a
            else:
                a = a.reshape(-1)
                if a.size and a.dtype.kind not in "iu":
                    raise ValueError(f"scene {b}: row indices must be integers, got {a.dtype}")
                if a.size and (int(a.min()) < 0 or int(a.max()) >= nb):
                    raise ValueError(f"scene {b}: row indices must lie in 0 .. {nb - 1}")
                out[so[b] + a.astype(np.int64)] = 1
        return out
    a = np.asarray(mask)
    if a.dtype.kind not in "bu" or a.shape != (n,):
        raise ValueError(f"a mask over the concatenated rows must be bool (or uint8) of shape ({n},), got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a != 0, dtype=np.uint8)


def heading32(x, y, vx, vy, wx, wy):
    """The heading of frame 1, per row, in the kernel's fp32 arithmetic: v / |v| when fmaf(vx, vx, vy * vy) > 0, else the goal
    entry (wx - x, wy - y) / its length when that is > 0, else (1, 0); l = sqrt(.), h = (a / l, b / l), each rounded once.
    ``observe.heading`` is the same rule with a float64 division, for tests that compare within a tolerance."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        gx, gy = wx - x, wy - y
        vv, gg = _fma32(vx, vx, vy * vy), _fma32(gx, gx, gy * gy)
        use_v = vv > 0
        use_g = ~use_v & (gg > 0)
        a = np.where(use_v, vx, gx)
        b = np.where(use_v, vy, gy)
        l = np.sqrt(np.where(use_v, vv, gg).astype(np.float32))
        hx = np.where(use_v | use_g, (a / l).astype(np.float32), np.float32(1.0)).astype(np.float32)
        hy = np.where(use_v | use_g, (b / l).astype(np.float32), np.float32(0.0)).astype(np.float32)
    return hx, hy


# The rules of the two scans, each stated once: the three lengths (_check_radii), the pruning test (_far), the per-disc arithmetic
# (_disc_ranges) and the choice of the first minimum (_first_minimum).  ``_walk`` casts from the rows, ``scan_vehicles_scene`` from
# the vehicles.

def _check_radii(max_range, ped_radius, point_radius):
    """The scan's three lengths as the library takes them -> (Rmax, ped_r2, point_r2) float32; raises ValueError."""
    Rmax = np.float32(max_range)
    if not (np.isfinite(Rmax) and 0 < Rmax <= np.float32(MAX_SCAN_RANGE)):
        raise ValueError(f"max_range must be finite, > 0 and <= {MAX_SCAN_RANGE:g} metres")
    for name, r in (("ped_radius", ped_radius), ("point_radius", point_radius)):
        if not (np.isfinite(np.float32(r)) and 0 <= np.float32(r) <= np.float32(MAX_SCAN_RANGE)):
            raise ValueError(f"{name} must be finite, >= 0 and <= {MAX_SCAN_RANGE:g} metres")
    return Rmax, radius2(ped_radius), radius2(point_radius)


def _far(ax, ay, r2, Rmax):
    """``scan_scene``'s pruning test: which candidates (offsets ax, ay from the origin, radius^2 r2) lie further than
    1.001 (Rmax + 2 r) from it."""
    d = np.sqrt(ax.astype(np.float64) ** 2 + ay.astype(np.float64) ** 2)
    return d > 1.001 * (np.float64(Rmax) + 2.0 * np.sqrt(r2.astype(np.float64))) + 1e-30


def _disc_ranges(ax, ay, r2, rx, ry):
    """The per-disc rules of include/sfm_hip.h for P discs (offsets ax, ay from the origin and r2, each (P,)) against R rays
    (rx, ry, each (R,)): (R, P) float32, the range of every candidate and +inf where the disc is no candidate of the ray."""
    A, Bv = ax[None, :], ay[None, :]
    U, V = rx[:, None], ry[:, None]
    t = _fma32(A, U, Bv * V)
    c = _fma32(A, V, -(Bv * U))
    q = _fma32(-c, c, r2[None, :])
    w = np.sqrt(q)
    cand = (q > 0) & ((t + w) > 0)
    s = t - w
    return np.where(cand, np.where(s > 0, s, np.float32(0.0)), np.float32(np.inf)).astype(np.float32)


def _first_minimum(val, kind, Rmax):
    """A ray's value from its candidates' ranges val (R, P) in the fixed order: (ranges (R,), kinds (R,)) float32."""
    R = val.shape[0]
    if val.shape[1] == 0:
        return np.full(R, Rmax, np.float32), np.zeros(R, np.float32)
    idx = np.argmin(val, axis=1)                                       # the first minimum in the fixed order
    best = val[np.arange(R), idx]
    hit = best < Rmax
    return np.where(hit, best, Rmax).astype(np.float32), np.where(hit, kind[idx].astype(np.float32), np.float32(0.0))


def _walk(scene, angles, max_range, ped_radius, point_radius, frame, mask, state, vehicles, waypoints, directions, prune):
    """The shared walk of ``scan_scene`` and ``range_census``: validates, then yields first (n, R, Rmax) and after it, per scanned
    live row in ascending order, (i, val, kind): val (R, P) float32 the range of every candidate in the fixed order (+inf where
    the disc is no candidate of the ray), kind (P,) int64."""
    if frame not in (0, 1):
        raise ValueError(f"frame must be 0 or 1, got {frame!r}")
    ux, uy = ray_directions(angles) if directions is None else check_directions(directions)
    R = ux.shape[0]
    Rmax, pr2, qr2 = _check_radii(max_range, ped_radius, point_radius)
    loc, vel = (_get(scene, "loc"), _get(scene, "vel")) if state is None else state
    loc, vel = np.asarray(loc, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    yield n, R, Rmax
    if n == 0:
        return
    loc, vel = loc.reshape(n, -1), vel.reshape(n, -1)
    x, y = _f32(loc[:, 0], 0), _f32(loc[:, 1], 0)
    vx, vy = _f32(vel[:, 0], 0), _f32(vel[:, 1], 0)
    scanned = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool).reshape(n)
    live = _live(x, y)
    if frame == 1:
        wp = np.asarray(_get(scene, "waypoint") if waypoints is None else waypoints, dtype=np.float64).reshape(n, -1)
        hx, hy = heading32(x, y, vx, vy, _f32(wp[:, 0], 0), _f32(wp[:, 1], 0))

    borders = _get(scene, "borders") or []
    statics = _get(scene, "static_obstacles") or []
    veh = (_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles
    geo = [_polylines(borders, False)[0], _polylines(statics, True)[0], _polylines(veh, True)[0]]
    gx = np.concatenate([g[:, 0] for g in geo])
    gy = np.concatenate([g[:, 1] for g in geo])
    gkind = np.concatenate([np.full(len(g), KIND_BORDER + q, np.int64) for q, g in enumerate(geo)])
    can_prune = bool(prune) and bool((np.abs(ux.astype(np.float64) ** 2 + uy.astype(np.float64) ** 2 - 1.0) < 1e-6).all())

    with np.errstate(over="ignore", invalid="ignore"):
        for i in np.flatnonzero(scanned & live):
            others = np.arange(n) != i
            px = np.concatenate([x[others], gx])
            py = np.concatenate([y[others], gy])
            r2 = np.concatenate([np.full(n - 1, pr2, np.float32), np.full(len(gx), qr2, np.float32)])
            kind = np.concatenate([np.full(n - 1, KIND_PEDESTRIAN, np.int64), gkind])
            ax, ay = px - x[i], py - y[i]
            keep = r2 > 0                                              # (radius 0: q = -c^2 <= 0, never a candidate)
            if can_prune:
                keep &= ~_far(ax, ay, r2, Rmax)
            if frame == 1:
                rx = _fma32(hx[i], ux, -(hy[i] * uy))
                ry = _fma32(hy[i], ux, hx[i] * uy)
            else:
                rx, ry = ux, uy
            yield i, _disc_ranges(ax[keep], ay[keep], r2[keep], rx, ry), kind[keep]


def scan_scene(scene, angles, max_range, ped_radius, point_radius, frame=0, mask=None, state=None, vehicles=None, waypoints=None,
               directions=None, prune=True):
    """The scan record of one scene, (N, 2R) float32, as ``SfmBatch.scans()`` returns it: floats 0 .. R-1 the ranges, R .. 2R-1
    the kinds (0 nothing, 1 pedestrian, 2 border, 3 static obstacle, 4 vehicle).

    ``scene``: a scene dict as ``SfmBatch.upload`` takes it (or a ``scenarios.Scenario``).  ``angles``: the R ray angles (see
    ``ray_directions``; ``default_angles(R)`` is ``set_scan``'s default), or None with ``directions`` = (dir_x, dir_y) used as
    given.  ``max_range``, ``ped_radius``, ``point_radius``: metres, this scene's.  ``frame``: 0 world axes, 1 heading frame.
    ``mask``: bool (N,), the rows that are scanned (None: all).  What has changed on the device since the upload is fed in as for
    ``observe.observe_scene``: ``state`` = (loc, vel), ``vehicles`` = the scene's list of (center, ring), ``waypoints`` (N,2|3).

    Chunked per row: the largest block is R x (N - 1 + points).  ``prune``: candidates further than 1.001 (Rmax + 2 r) from the row
    are left out before the ray arithmetic when every direction has | |u|^2 - 1 | < 1e-6.  That cannot change the record: a
    candidate needs q > 0, so |c| <= r up to rounding and t >= |a||u| - r up to rounding (2^-22 |a| each), hence its range
    t - w >= |a| (1 - 1.3e-6) - 2.0000002 r > Rmax, and a range >= Rmax is never stored (if it is the minimum the ray is a miss;
    if it is not, it is not the minimum).  ``prune=False`` evaluates everything."""
    walk = _walk(scene, angles, max_range, ped_radius, point_radius, frame, mask, state, vehicles, waypoints, directions, prune)
    n, R, Rmax = next(walk)
    rec = np.zeros((n, 2 * R), np.float32)
    for i, val, kind in walk:
        rec[i, :R], rec[i, R:] = _first_minimum(val, kind, Rmax)
    return rec


def range_census(scene, angles, max_range, ped_radius, point_radius, frame=0, mask=None, state=None, vehicles=None, waypoints=None,
                 directions=None, band=0.01):
    """How hard a scene tests the range limit: an int64 array (5, 2), per kind the number of (row, ray, candidate) triples whose
    range lies in [(1 - band) Rmax, Rmax) and in [Rmax, (1 + band) Rmax] -- just inside and just outside the limit.  Arguments as
    for ``scan_scene``; nothing is pruned."""
    walk = _walk(scene, angles, max_range, ped_radius, point_radius, frame, mask, state, vehicles, waypoints, directions, False)
    _, _, Rmax = next(walk)
    lo, hi = np.float64(Rmax) * (1.0 - band), np.float64(Rmax) * (1.0 + band)
    out = np.zeros((5, 2), np.int64)
    for _, val, kind in walk:
        v = val.astype(np.float64)
        for k in range(1, 5):
            vk = v[:, kind == k]
            out[k, 0] += int(((vk >= lo) & (vk < Rmax)).sum())
            out[k, 1] += int(((vk >= Rmax) & (vk <= hi)).sum())
    return out


# What follows is the vehicles' scan, built from the same pieces.

def check_mount(mount):
    """The sensor's place in the vehicle frame (x forward), metres -> (mx, my) float32; finite, |m| <= 1e6.  Raises ValueError."""
    try:
        mx, my = mount
        with np.errstate(over="ignore", invalid="ignore"):
            mx, my = np.float32(mx), np.float32(my)
    except (TypeError, ValueError):
        raise ValueError("mount must be a pair (x, y) of numbers") from None
    if not (np.isfinite(mx) and np.isfinite(my) and abs(mx) <= np.float32(MAX_SCAN_RANGE) and abs(my) <= np.float32(MAX_SCAN_RANGE)):
        raise ValueError(f"mount must be finite and within {MAX_SCAN_RANGE:g} metres of the vehicle's centre")
    return mx, my


def vehicle_scan_origin(center, heading, mount):
    """The sensor's origin by the rule of include/sfm_hip.h, all fp32: (cx + fmaf(hx, mx, -(hy my)), cy + fmaf(hy, mx, hx my))."""
    cx, cy = np.float32(center[0]), np.float32(center[1])
    hx, hy = np.float32(heading[0]), np.float32(heading[1])
    mx, my = np.float32(mount[0]), np.float32(mount[1])
    with np.errstate(over="ignore", invalid="ignore"):
        rx = _fma32(hx, mx, -(hy * my))[()]
        ry = _fma32(hy, mx, hx * my)[()]
        return np.float32(cx + rx), np.float32(cy + ry)


def scan_vehicles_scene(scene, angles, max_range, ped_radius, point_radius, frame=0, mask=None, mount=(0.0, 0.0), state=None,
                        vehicles=None, headings=None, directions=None, prune=True):
    """The vehicle scan record of one scene, (M_b, 2R) float32, as ``SfmBatch.vehicle_scans()`` returns it -- bit for bit in both
    frames (include/sfm_hip.h specifies the record): floats 0 .. R-1 the ranges, R .. 2R-1 the kinds.  Per scanned present vehicle R
    rays from the sensor's origin (the centre plus the mount turned by the stored heading); the candidates in the fixed order are
    EVERY pedestrian row, the border points, the static-obstacle points and the ring points of the scene's OTHER vehicles.

    ``scene``, ``angles`` / ``directions`` (1 .. 256 rays), ``max_range``, ``ped_radius``, ``point_radius``, ``frame`` and
    ``prune`` as for ``scan_scene``; ``mask`` (M_b,) bool, the vehicles that are scanned (None: all); ``mount`` = (x, y) in the
    vehicle frame.  What has changed on the device since the upload is fed in: ``state`` = (loc, vel) of the rows, ``vehicles`` =
    the scene's list of (center, ring), ``headings`` (M_b, 2) fp32 {cos, sin} (default: ``scenarios.vehicle_headings(scene)``, what
    the upload derives from ``dynamic_yaw``)."""
    from .scenarios import vehicle_headings
    if frame not in (0, 1):
        raise ValueError(f"frame must be 0 or 1, got {frame!r}")
    ux, uy = (ray_directions(angles, MAX_VEHICLE_SCAN_RAYS) if directions is None
              else check_directions(directions, MAX_VEHICLE_SCAN_RAYS))
    R = ux.shape[0]
    Rmax, pr2, qr2 = _check_radii(max_range, ped_radius, point_radius)
    mount = check_mount(mount)
    veh = list((_get(scene, "dynamic_obstacles") or []) if vehicles is None else vehicles)
    M = len(veh)
    if mask is None:
        scanned = np.ones(M, bool)
    else:
        scanned = np.asarray(mask)
        if scanned.shape != (M,):
            raise ValueError(f"a mask of shape {scanned.shape} for {M} vehicles")
        scanned = scanned != 0
    rec = np.zeros((M, 2 * R), np.float32)
    if M == 0:
        return rec
    h = _f32(vehicle_headings(scene) if headings is None else headings, 2)
    if h.shape != (M, 2):
        raise ValueError(f"headings of shape {h.shape} for {M} vehicles")
    loc = np.asarray(_get(scene, "loc") if state is None else state[0], dtype=np.float64)
    n = loc.reshape(-1, loc.shape[-1]).shape[0] if loc.size else 0
    loc = loc.reshape(n, -1) if n else np.zeros((0, 3))
    x, y = _f32(loc[:, 0], 0), _f32(loc[:, 1], 0)
    ctr = np.stack([_f32(c, 0)[:2] for c, _ in veh])
    rings = [_f32(r, 2) for _, r in veh]
    bpts = _polylines(_get(scene, "borders") or [], False)[0]
    spts = _polylines(_get(scene, "static_obstacles") or [], True)[0]
    can_prune = bool(prune) and bool((np.abs(ux.astype(np.float64) ** 2 + uy.astype(np.float64) ** 2 - 1.0) < 1e-6).all())
    with np.errstate(over="ignore", invalid="ignore"):
        for k in np.flatnonzero(scanned & _live(ctr[:, 0], ctr[:, 1])):
            ox, oy = vehicle_scan_origin(ctr[k], h[k], mount)
            other = [rings[v] for v in range(M) if v != k] + [np.zeros((0, 2), np.float32)]
            geo = [bpts, spts, np.concatenate(other, axis=0)]
            px = np.concatenate([x] + [g[:, 0] for g in geo])
            py = np.concatenate([y] + [g[:, 1] for g in geo])
            r2 = np.concatenate([np.full(n, pr2, np.float32), np.full(len(px) - n, qr2, np.float32)])
            kind = np.concatenate([np.full(n, KIND_PEDESTRIAN, np.int64)] + [np.full(len(g), KIND_BORDER + q, np.int64) for q, g in enumerate(geo)])
            ax, ay = px - ox, py - oy
            keep = r2 > 0                                              # (radius 0: q = -c^2 <= 0, never a candidate)
            if can_prune:
                keep &= ~_far(ax, ay, r2, Rmax)
            if frame == 1:
                rx = _fma32(h[k, 0], ux, -(h[k, 1] * uy))
                ry = _fma32(h[k, 1], ux, h[k, 0] * uy)
            else:
                rx, ry = ux, uy
            rec[k, :R], rec[k, R:] = _first_minimum(_disc_ranges(ax[keep], ay[keep], r2[keep], rx, ry), kind[keep], Rmax)
    return rec
