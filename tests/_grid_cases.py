"""Shared cases of the occupancy-grid tests (tests/test_batch_grid_host.py, tests/test_batch_grid_gpu.py): scene builders whose
coordinates are all fp32-representable, and a float64 statement of what the grid's bits mean.

What the bits mean
------------------
The record is defined by fp32 rules (include/sfm_hip.h); ``truth`` evaluates the same geometry in float64 from the same fp32
inputs: p* = rot(px - x, py - y) / c + G / 2 per axis, cell = floor(p*).  The two agree on the cell of a source unless p* lies
within a margin delta of an integer.  With u = 2^-24, the unit roundoff of fp32, and a source that is in range (|p* - G/2| <= G/2
on both axes, so |px - x| / c <= G / 2 per axis in frame 0 and |a| / c <= G / sqrt(2) for the vector a = (px - x, py - y) in frame 1,
a rotation keeping the norm):

frame 0, operation by operation
    ax = fl(px - x)            relative error <= u                      (inputs are exact fp32)
    q  = fl(ax / c)            another u: |q - q*| <= (2u + u^2) |q*| <= (G/2)(2u + u^2)
    pu = fl(q + half)          another u of |pu| <= G: <= G u (1 + 2u)
    sum: |pu - p*| <= 2 G u + O(u^2);  DELTA[0] = 2.5 G u.

frame 1, the heading first
    vv = fmaf(vx, vx, fl(vy * vy)): two roundings of non-negative terms, relative <= 2u; l = fl(sqrt(vv)): the root halves that
    to u and rounds once more, <= 2u; hx = fl(vx / l): <= 3u + O(u^2)
    from the goal: gx = fl(wx - x), gy likewise, u each: the direction's components move by <= 2u more: <= 5u + O(u^2) =: e_h
    fx = fmaf(hx, ax, fl(hy * ay)):
        hx ax           carries e_h + u (ax)                <= 6u |ax|
        fl(hy ay)       carries e_h + u (ay) + u (product)  <= 7u |ay|
        the fma's rounding                                  <= u |fx| <= u |a|
        |fx - fx*| <= 7u (|ax| + |ay|) + u |a| <= (7 sqrt(2) + 1) u |a| < 11 u |a|, and |a| / c <= G / sqrt(2): <= 7.8 G u in cells
    then the division and the sum as in frame 0: + 1.5 G u + O(u^2)
    sum: |pu - p*| <= 9.3 G u + O(u^2);  DELTA[1] = 12 G u.
float64's own rounding of p* (2^-53 relative) disappears in the slack.  ``truth`` takes the twin's DECISION of which vector gives the
heading (fmaf(vx, vx, vy * vy) > 0 in fp32, then the goal, then (1, 0)) and normalises that vector in float64: an underflowing |v|^2
is a case the rule decides, not an error of rounding.

Velocity sums.  A term is t = rot(v_j - v): the difference carries u, the rotation (as fx above) < 11 u |t|; use 12 u |t| in both
frames.  k terms added one after the other in fp32 add at most (k - 1) u sum |t_j| / (1 - (k - 1) u) (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2).  ``SUM_BOUND(k, s)`` = (k + 12) u s 1.001 with s = sum_j |t_j|_2 bounds both.
"""
import numpy as np

from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd.observe import NEAR_LIMIT
from carla_social_force_model_amd.scan import _fma32

U = 2.0 ** -24
TILE = 1024                          # GRID_TILE of sfm_batch_grid.hip: the geometry points the kernel's LDS tile holds
f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)      # a float64 array of fp32-representable values


def delta(G, frame):
    return (12.0 if frame else 2.5) * G * U


def sum_bound(k, s):
    return (k + 12) * U * s * 1.001


def tiny(loc, vel=None, waypoint=None, borders=(), statics=(), vehicles=()):
    """A scene dict of a few hand-placed rows: what the twin reads (and what SfmBatch.upload needs)."""
    loc = f32(np.asarray(loc, dtype=np.float64).reshape(-1, 2))
    n = len(loc)
    z = np.zeros((n, 1))
    vel = np.zeros((n, 2)) if vel is None else f32(np.asarray(vel, dtype=np.float64).reshape(n, 2))
    wp = loc.copy() if waypoint is None else f32(np.asarray(waypoint, dtype=np.float64).reshape(n, 2))
    borders = [f32(b).reshape(-1, 2) for b in borders]
    ring = lambda pts: (np.zeros(2), f32(pts).reshape(-1, 2))            # (the centre is not read by the grids)
    return {"loc": np.hstack([loc, z]), "vel": np.hstack([vel, z]), "waypoint": np.hstack([wp, z]),
            "target_speed": np.full(n, 1.25), "radius": np.full(n, 0.25),
            "borders": borders, "border_centers": np.array([b[len(b) // 2] for b in borders]).reshape(-1, 2),
            "border_lengths": np.array([0.1 * len(b) for b in borders], dtype=np.float64),
            "static_obstacles": [ring(p) for p in statics], "dynamic_obstacles": [ring(p) for p in vehicles],
            "dynamic_vel": np.zeros((len(vehicles), 2)), "dynamic_yaw": np.zeros(len(vehicles)),
            "dynamic_extent": np.tile([2.4, 1.0], (len(vehicles), 1)).reshape(-1, 2)}


def crowd(n, seed, points=None, dynamic=0):
    """A generated scene of n rows (a jittered lattice, about 2 m apart).  ``points``: None -- 6 borders, 3 static obstacles and
    ``dynamic`` vehicles as generated; else exactly that many geometry points in all: the static rings and vehicles as generated
    (when they fit) and ONE border through the crowd that holds the rest."""
    geo = points is None or points > 0
    sc = vars(scenarios.make_scenario(n, seed, n_borders=6 if points is None else 0, n_static=3 if geo else 0, n_dynamic=dynamic if geo else 0,
                                      border_len=(3.0, 15.0)))
    if points is not None and points > 0:
        have = sum(len(r) for _, r in sc["static_obstacles"]) + sum(len(r) for _, r in sc["dynamic_obstacles"])
        if have > points - 1:
            sc["static_obstacles"], have = [], sum(len(r) for _, r in sc["dynamic_obstacles"])
        k = points - have
        assert k >= 1
        side = max(float(sc["world_side"]), 4.0)
        t = np.arange(k)
        # a zigzag across the crowd: 1/16 m steps along x (wrapped), rows 1/4 m apart -- all exact in fp32
        line = f32(np.column_stack(((t % int(side * 16)) / 16.0, 0.5 + (t // int(side * 16)) / 4.0)))
        sc["borders"] = [line]
        sc["border_centers"] = line[len(line) // 2].reshape(1, 2)
        sc["border_lengths"] = np.array([0.1 * k])
    sc["radius"] = f32(np.random.default_rng(seed + 17).uniform(0.2, 0.45, n))
    return sc


def geometry_points(sc):
    return (sum(len(b) for b in sc["borders"]) + sum(len(r) for _, r in sc["static_obstacles"]) +
            sum(len(r) for _, r in sc["dynamic_obstacles"]))


# ---- the mixed batch of the device tests ----------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 0, 65, 257, 1024)
POINTS = (0, TILE - 1, TILE, TILE + 1, None, 3 * TILE + 17, None, None)          # None: as generated (the last two with vehicles)
CELLS = (0.5, 1.0, 0.75, 2.0, 1.0, 0.3125, 0.5, 1.5)                             # metres, per scene
GS = (1, 2, 15, 16, 17, 32)


def mixed_batch():
    """Scenes of 1, 2, 63, 64, 0 (empty), 65, 257 and 1 024 rows; geometry of 0, TILE - 1, TILE, TILE + 1 and several tiles of
    points; dead rows: one parked far away (a ghost) in the scenes of 63, 257 and 1 024 rows."""
    scenes = [crowd(n, 6100 + q, p, dynamic=3 if q >= 6 else 0) for q, (n, p) in enumerate(zip(SIZES, POINTS))]
    for q, row in ((2, 5), (6, 200), (7, 1000)):
        scenes[q]["loc"] = np.array(scenes[q]["loc"])
        scenes[q]["loc"][row, :2] = 4.0e12
    for sc, p in zip(scenes, POINTS):
        assert p is None or geometry_points(sc) == p
    return scenes


def masks(kind, sizes=SIZES):
    """The row masks of the device tests, as SfmBatch.set_grid takes them: None; "agent" -- one row per scene (the last);
    "all" -- every row, spelled out; "holes" -- every third row, and none at all of the 64-row scene."""
    if kind is None:
        return None
    out = []
    for n in sizes:
        m = np.zeros(n, bool)
        if kind == "agent" and n:
            m[n - 1] = True
        elif kind == "all":
            m[:] = True
        elif kind == "holes" and n != 64:
            m[1::3] = True
        out.append(m)
    return out


# ---- one source per owning wave: the accumulation's wave test ---------------------------------------------------------------------
BLOCK, WAVE = 256, 64                # sfm_device.h: a lane owns the cells tid + q BLOCK; cell id's owning wave is (id / WAVE) % 4
BIG = 2.0 ** 25
ORDER_VALUES = (1.0, -BIG, BIG)      # (_vehicle_grid_cases.ORDER_VALUES) added in this order the fp32 sum is 0; with the 1 last it is 1
WAVE_CELLS = {32: ([WAVE * w + BLOCK * q + l for w in range(4) for q in range(4) for l in (0, WAVE - 1)], [WAVE * w for w in range(4)]),
              8: ([0, 7, 27, 36, 56, 63], [27])}       # G: (the cells that are hit, those of them that hold the order triple)


def wave_scene(G):
    """(scene, expected): row 0 stands at the fp32 origin, goal straight ahead along +x, and is the one gridded row; every cell of
    WAVE_CELLS[G][0] of its 1 m grid holds one source at the cell's centre with a velocity of its own, and the cells of
    WAVE_CELLS[G][1] three, a quarter cell apart, whose x-velocities are ORDER_VALUES in row order.  ``expected``:
    {cell: (count, sum vx, sum vy)}, stated by hand.  Every coordinate is a multiple of 1/4 and so exact in fp32; with heading
    (1, 0) frame 1 is frame 0."""
    hit, triple = WAVE_CELLS[G]
    loc, vel, expected = [(0.0, 0.0)], [(0.0, 0.0)], {}
    for cid in hit:
        x, y = cid % G - G / 2 + 0.5, cid // G - G / 2 + 0.5
        if cid in triple:
            loc += [(x - 0.25, y - 0.25), (x, y), (x + 0.25, y + 0.25)]
            vel += [(v, 0.0) for v in ORDER_VALUES]
            expected[cid] = (3.0, 0.0, 0.0)
        else:
            loc.append((x, y))
            vel.append((cid / 8.0, -1.0 - cid))
            expected[cid] = (1.0, cid / 8.0, -1.0 - cid)
    return tiny(loc, vel, waypoint=[(1.0, 0.0)] + loc[1:]), expected


# ---- float64 truth --------------------------------------------------------------------------------------------------------------

def _heading64(x, y, vx, vy, wx, wy):
    """The heading of frame 1 in float64, with the twin's fp32 decision of which vector gives it."""
    gx, gy = np.float32(wx) - np.float32(x), np.float32(wy) - np.float32(y)
    with np.errstate(all="ignore"):
        use_v = _fma32(vx, vx, np.float32(vy) * np.float32(vy)) > 0
        use_g = _fma32(gx, gx, gy * gy) > 0
    if use_v:
        a, b = np.float64(vx), np.float64(vy)
    elif use_g:
        a, b = np.float64(wx) - np.float64(x), np.float64(wy) - np.float64(y)
    else:
        return 1.0, 0.0
    l = np.hypot(a, b)
    return a / l, b / l


def truth(scene, G, cell, frame, row):
    """Float64 view of gridded row ``row`` of a scene dict: a list of 4 entries (pedestrians, borders, static, vehicles), each
    (pu, pv) float64 arrays of the kind's sources (pedestrians: live rows j != row, ascending), and the pedestrians' relative
    velocities (tx, ty) in the grid's frame."""
    loc, vel, wp = (np.asarray(scene[k], dtype=np.float64) for k in ("loc", "vel", "waypoint"))
    x, y = f32(loc[:, 0]), f32(loc[:, 1])
    vx, vy = f32(vel[:, 0]), f32(vel[:, 1])
    c = np.float64(np.float32(cell))
    hx, hy = _heading64(x[row], y[row], vx[row], vy[row], f32(wp[row, 0]), f32(wp[row, 1])) if frame else (1.0, 0.0)
    with np.errstate(all="ignore"):
        alive = (np.abs(x) < NEAR_LIMIT) & (np.abs(y) < NEAR_LIMIT)
    src = alive.copy()
    src[row] = False
    ring = lambda items: np.concatenate([f32(r).reshape(-1, 2) for _, r in items]) if items else np.zeros((0, 2))
    kinds = [np.column_stack((x[src], y[src])),
             np.concatenate([f32(b).reshape(-1, 2) for b in scene["borders"]]) if len(scene["borders"]) else np.zeros((0, 2)),
             ring(scene["static_obstacles"]), ring(scene["dynamic_obstacles"])]
    out = []
    with np.errstate(all="ignore"):
        for p in kinds:
            ax, ay = p[:, 0] - x[row], p[:, 1] - y[row]
            out.append(((hx * ax + hy * ay) / c + G / 2.0, (hx * ay - hy * ax) / c + G / 2.0))
        rx, ry = vx[src] - vx[row], vy[src] - vy[row]
    return out, (hx * rx + hy * ry, hx * ry - hy * rx)


def classify(pu, pv, G, d):
    """Per source: (certain, cell) -- ``certain``: the float64 coordinates are further than d from every integer on both axes, or
    clearly out of range; ``cell``: floor's cell id cv * G + cu, -1 out of range.  An uncertain source lies in the margin."""
    with np.errstate(all="ignore"):
        near = lambda p: (np.abs(p - np.round(p)) <= d) & (p >= -d) & (p <= G + d)
        inside = (pu >= 0) & (pu < G) & (pv >= 0) & (pv < G)
        fin = np.isfinite(pu) & np.isfinite(pv)
        # a source beyond the grid on one axis is outside whatever the other axis says
        away = ~fin | (pu < -d) | (pu > G + d) | (pv < -d) | (pv > G + d)
        certain = away | ~(near(pu) | near(pv))
        cu = np.where(inside & fin, np.floor(np.where(fin, pu, 0.0)), 0).astype(np.int64)
        cv = np.where(inside & fin, np.floor(np.where(fin, pv, 0.0)), 0).astype(np.int64)
    return certain, np.where(inside & fin, cv * G + cu, -1)
