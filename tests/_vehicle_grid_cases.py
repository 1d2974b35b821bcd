"""Shared cases of the vehicle-grid tests (tests/test_batch_vehicle_grid_host.py, tests/test_batch_vehicle_grid_gpu.py): hand-placed
scenes whose coordinates are all fp32-representable, the mixed batch the device tests run, and a float64 statement of what the
record's bits mean.

What the bits mean
------------------
The record is defined by fp32 rules (include/sfm_hip.h); ``truth`` evaluates the same geometry in float64 from the same fp32 inputs
and the stored heading used as given: o* = c + R(h) m, a* = p - o*, f* = a* (frame 0) or R(h)^T a* (frame 1), pu* = fx* / c + GU / 2,
pv* = fy* / c + GV / 2, cell = floor.  The two agree on the cell of a source unless pu* or pv* lies within a margin of an integer.
With u = 2^-24, H = max(|hx|, |hy|, 1) and m = |mx| + |my|, operation by operation for ONE source:

    hy my, hx my            one rounding each                                <= u |h| |m_i|
    rx = fmaf(hx, mx, .)    one more of |rx| <= H m                          |rx - rx*| <= 2 u H m
    ox = fl(cx + rx)        one more of |ox|                                 e_o = u (|ox| + 2 H m), and likewise oy
        -- ABSOLUTE in metres: it grows with the scene's extent, not with the window, and costs e_o / c cells.  The case scenes keep
           their coordinates within a few hundred metres, so e_o / c stays near 1e-5 cells.
    ax = fl(px - ox)        one rounding of |ax|, and o's error               e_a = u A + e_o,  A = max(|ax*|, |ay*|)
    frame 1: fx = fmaf(hx, ax, fl(hy ay))
        fl(hy ay)           u |hy ay| <= u H A
        the fma's rounding  u |fx| <= 2 u H A
        the inputs' errors  (|hx| + |hy|) e_a <= 2 H e_a                     e_f = 3 u H A + 2 H e_a     (frame 0: e_f = e_a)
    q = fl(fx / c)          u |q| <= 2 u H A / c, and e_f / c
    pu = fl(q + half)       u |pu| <= u (2 H A / c + G / 2)
    sum: |pu - pu*| <= e_f / c + 4 u H A / c + u G / 2 =: ``margin`` (with 1 % of slack for the terms in u^2), G = max(GU, GV).
A source far outside the window has a large A and so a large margin of its own, but stays outside by more than that: the margin
is relative to A there.  float64's own rounding of pu* (2^-53 relative) disappears in the slack.

Outside the margin the twin's cell is floor's.  Inside it the source may sit in a neighbouring cell (or on the other side of the
window's edge): with U_k uncertain sources of a kind, the counts of the certain sources are a lower bound cell by cell and at most
U_k more are counted in all.  The case scenes are chosen so that at most 1 % of the in-range sources of any of them lie in the
margin (the cap tests/test_batch_grid_host.py uses), which the host test checks of the twin alone.

Velocity sums.  A term is t = rot(v_j - v_k): the difference carries u, the rotation (as fx above, with the heading exact) <= 3 u H |t|;
use 12 u |t| as tests/_grid_cases.py does.  k terms added one after the other in fp32 add at most (k - 1) u sum |t_j| (1 + O(k u)).
``sum_bound(k, s)`` = (k + 12) u s 1.001 with s = sum_j |t_j|_1 bounds both.
"""
import copy
from functools import lru_cache

import numpy as np

from carla_social_force_model_amd import grid as G, scenarios
from carla_social_force_model_amd.observe import NEAR_LIMIT

U = 2.0 ** -24
TILE, LIST, BLOCK = 1024, 512, 256                   # sfm_batch_vehicle_grid.hip: points per LDS tile, list entries per chunk, lanes
f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)      # a float64 array of fp32-representable values
ZERO, FORWARD = (0.0, 0.0), (3.0, -0.5)


def sum_bound(k, s):
    return (k + 12) * U * s * 1.001


# ---- hand-placed scenes ---------------------------------------------------------------------------------------------------------

def hand(peds=(), vels=None, vehicles=((0.0, 0.0),), vehicle_vel=None, yaw=None, extent=(0.5, 0.25), borders=(), statics=()):
    """A scene dict of hand-placed rows and boxes: what the twin reads and what SfmBatch.upload(device_vehicles=True) needs.  The
    rings are the boxes' own (``scenarios.place_ring_f32``), as the device forms them."""
    loc = f32(np.asarray(peds, dtype=np.float64).reshape(-1, 2))
    n, M = len(loc), len(vehicles)
    z = np.zeros((n, 1))
    vel = np.zeros((n, 2)) if vels is None else f32(np.asarray(vels, dtype=np.float64).reshape(n, 2))
    yaw = np.zeros(M) if yaw is None else np.asarray(yaw, dtype=np.float64).reshape(M)
    ext = np.broadcast_to(np.asarray(extent, dtype=np.float64), (M, 2)).copy()
    ctr = f32(np.asarray(vehicles, dtype=np.float64).reshape(M, 2))
    borders = [f32(b).reshape(-1, 2) for b in borders]
    sc = {"loc": np.hstack([loc, z]), "vel": np.hstack([vel, z]), "waypoint": np.hstack([loc + 1.0, z]),
          "target_speed": np.full(n, 1.25), "radius": np.full(n, 0.25),
          "borders": borders, "border_centers": np.array([b[len(b) // 2] for b in borders]).reshape(-1, 2),
          "border_lengths": np.array([0.1 * len(b) for b in borders], dtype=np.float64),
          "static_obstacles": [(f32(p).reshape(-1, 2).mean(axis=0), f32(p).reshape(-1, 2)) for p in statics],
          "dynamic_obstacles": [(ctr[k], None) for k in range(M)],
          "dynamic_vel": np.zeros((M, 2)) if vehicle_vel is None else f32(np.asarray(vehicle_vel, dtype=np.float64).reshape(M, 2)),
          "dynamic_yaw": yaw, "dynamic_extent": ext}
    sc["dynamic_obstacles"] = [(ctr[k], scenarios.place_ring_f32(ctr[k], yaw[k], scenarios.ring_local_offsets(*ext[k]))) for k in range(M)]
    return sc


BIG = 2.0 ** 25
ORDER_VALUES = (1.0, -BIG, BIG)      # added in this order: fl(1 - 2^25) = -2^25, then 0; in any other order the sum is 1 or more


def ordered(values):
    """The fp32 sum of ``values`` added one after the other from 0.0f."""
    s = np.float32(0.0)
    for v in values:
        s = np.float32(s + np.float32(v))
    return s


def order_scene_pedestrians(values=ORDER_VALUES):
    """Three pedestrians in one cell (a 1 m cell around (2.5, 0.5)) whose x-velocities are ``values``; the vehicle stands."""
    return hand(peds=[(2.25, 0.25), (2.5, 0.5), (2.75, 0.75)], vels=[(v, 0.0) for v in values])


def order_scene_vehicles(values=ORDER_VALUES):
    """Three small vehicles in one cell (their rings are 6 points within 2 cm of the centres) whose x-velocities are ``values``,
    seen from vehicle 0, which stands at the origin."""
    ctr = [(0.0, 0.0), (2.25, 0.25), (2.5, 0.5), (2.75, 0.75)]
    return hand(vehicles=ctr, vehicle_vel=[(0.0, 0.0)] + [(v, 0.0) for v in values], extent=[(0.5, 0.25)] + [(0.01, 0.01)] * 3)


# ---- the mixed batch of the device tests ----------------------------------------------------------------------------------------
SIZES = (17, 0, 1, 255, 256, 257, 1024, 64, 17)       # pedestrians per scene
COUNTS = (0, 2, 1, 2, 9, 3, 2, 70, 3)                 # vehicles per scene
CELLS = (0.5, 0.5, 0.25, 0.5, 0.75, 0.5, 1.0, 0.5, 0.5)      # metres, per scene
DTS = [0.05, 0.04, 0.02, 0.05, 0.03, 0.05, 0.05, 0.04, 0.05]
GHOST, NAN_ROW = 3, 7                                 # rows of scene 5
ABSENT = (4, 4)                                       # (scene, vehicle): tracked, first tick 40
CROWDED, STRADDLE = 7, 8                              # the scene of 70 small vehicles; the scene whose vehicle 0 straddles the tile
# which vehicles are gridded: per name one entry per scene; "all" is no mask at all (a NULL pointer for the library)
_one = lambda m, k: [int(j == k) for j in range(m)]
MASKS = {"all": [None] * 9,
         "first": [_one(m, 0) for m in COUNTS],
         "middle": [_one(m, m // 2) if s not in (3, 6) else [0] * m for s, m in enumerate(COUNTS)],     # scenes 3 and 6: none
         "last": [_one(m, m - 1) for m in COUNTS]}
# what the GPU file runs -- GU, GV, cell scale, frame, centre, mask, planar: every window with both frames, both centres, every mask
# and both uploads somewhere
CASES = [(1, 1, 16.0, 0, ZERO, "all", None), (1, 1, 16.0, 1, FORWARD, "first", False), (17, 15, 1.0, 1, FORWARD, "first", None),
         (16, 16, 1.0, 0, FORWARD, "all", False), (33, 8, 1.0, 1, ZERO, "middle", None), (64, 16, 0.5, 1, FORWARD, "all", None),
         (32, 32, 1.0, 0, ZERO, "last", None), (32, 32, 0.5, 1, FORWARD, "all", None), (5, 64, 1.0, 1, FORWARD, "all", False),
         (5, 64, 1.0, 0, ZERO, "middle", None)]


def mask_arg(name):
    """The mask as set_vehicle_grid takes it."""
    return None if name == "all" else MASKS[name]


def counts(sc):
    """(border points, static points, ring sizes) of a scene."""
    return (sum(len(p) for p in sc["borders"]), sum(len(r) for _, r in sc["static_obstacles"]),
            [len(r) for _, r in sc["dynamic_obstacles"]])


def own_ring(sc, k):
    """Vehicle k's own ring as [lo, hi) of the geometry's virtual run (borders, static points, rings)."""
    nb, ns, rings = counts(sc)
    lo = nb + ns + sum(rings[:k])
    return lo, lo + rings[k]


@lru_cache(maxsize=None)
def _made():
    import test_batch_gpu as TB
    import test_batch_tracks_gpu as TR
    import test_batch_vehicles_gpu as V
    scenes = []
    for k, (n, m) in enumerate(zip(SIZES, COUNTS)):
        sc = TB._scene(n, 5200 + k, geo=k != 1, dynamic=m)
        rng = np.random.default_rng(950 + k)
        if k == CROWDED:                                                  # 70 small vehicles all over the crowd
            c = np.float32(sc["loc"][rng.integers(0, n, m), :2] + rng.uniform(-5.0, 5.0, (m, 2))).astype(np.float64)
            sc["dynamic_extent"] = np.tile([0.6, 0.3], (m, 1))
            sc["dynamic_obstacles"] = [(c[j], sc["dynamic_obstacles"][j][1]) for j in range(m)]
        elif m and n:                                                     # the vehicles stand inside the crowd
            c = np.float32(sc["loc"][rng.integers(0, n, m), :2] + rng.uniform(-1.5, 1.5, (m, 2))).astype(np.float64)
            sc["dynamic_obstacles"] = [(c[j], sc["dynamic_obstacles"][j][1]) for j in range(m)]
        elif m:                                                           # no crowd: two vehicles in sight of each other
            c = np.array([[2.0, 3.0], [6.0, 4.0]])
            sc["dynamic_extent"] = np.array([[3.0, 1.2], [1.6, 0.8]])
            sc["dynamic_obstacles"] = [(c[j], sc["dynamic_obstacles"][j][1]) for j in range(m)]
        sc["dynamic_vel"] = np.float32(sc["dynamic_vel"] * 0.1).astype(np.float64)
        V._restart_twin(sc)
        scenes.append(sc)
    sc = scenes[5]
    sc["loc"][GHOST, :2] = (3.0e15, -3.0e15)
    sc["vel"][GHOST] = 0.0
    sc["loc"][NAN_ROW, :2] = np.nan
    # the straddling scene: one more border through the crowd, so long that vehicle 0's own ring lies across the tile boundary
    sc = scenes[STRADDLE]
    nb, ns, rings = counts(sc)
    extra = TILE - rings[0] // 2 - (nb + ns)
    assert extra >= 2, "the straddling scene has too much geometry: choose another seed"
    t = np.arange(extra)
    mid = sc["loc"][:, :2].mean(axis=0)
    line = f32(np.column_stack((np.round(mid[0]) - 8.0 + (t % 256) / 16.0, np.round(mid[1]) - 1.0 + (t // 256) / 2.0)))
    sc["borders"] = list(sc["borders"]) + [line]
    sc["border_centers"] = np.vstack([np.asarray(sc["border_centers"]).reshape(-1, 2), line[len(line) // 2]])
    sc["border_lengths"] = np.concatenate([np.asarray(sc["border_lengths"]).reshape(-1), [0.1 * extra]])
    rng = np.random.default_rng(78)
    tracks = [None] * len(scenes)
    tracks[ABSENT[0]] = [None] * COUNTS[ABSENT[0]]
    tracks[ABSENT[0]][ABSENT[1]] = TR._track(rng, 5, 40, TR._mid(scenes[ABSENT[0]]))
    cfgs = [TB._config(k, scenarios.ALL_FORCES) for k in range(len(scenes))]
    return scenes, cfgs, tracks


def made(finite=False):
    """(scenes, configs, tracks), fresh copies; the twin of the batch as it is after upload(device_vehicles=True) and
    set_vehicle_tracks(tracks).  ``finite``: the NaN row is parked like the ghost (for tests that run ticks)."""
    import _driving_cases as D
    scenes, cfgs, tracks = copy.deepcopy(_made())
    if finite:
        scenes[5]["loc"][NAN_ROW, :2] = (3.0e15, 3.0e15)
    D.start_twin(scenes, tracks)
    return scenes, cfgs, tracks


def cells_of(scale):
    return [np.float32(c * scale) for c in CELLS]


def twin(scenes, GU, GV, scale, frame, centre, mask, **fed):
    """The record of every scene from the twin: a list of (m_b, 8, GV, GU) arrays.  ``fed``: per-scene lists of what
    ``grid.grid_vehicles_scene`` is fed (state, vehicles, headings, vehicle_vel)."""
    return [G.grid_vehicles_scene(sc, GU, GV, cells_of(scale)[s], frame=frame, mask=MASKS[mask][s], centre=centre,
                                  **{key: v[s] for key, v in fed.items()}) for s, sc in enumerate(scenes)]


# ---- float64 truth --------------------------------------------------------------------------------------------------------------

def truth(scene, GU, GV, cell, frame, centre, k, headings=None):
    """Float64 view of gridded vehicle ``k`` of a scene dict (None when it is not present): a list of 4 entries (pedestrians,
    borders, static points, the other vehicles' ring points, each in the record's order), each (pu, pv, margin) float64 arrays of
    the kind's sources, and the relative velocities (tx, ty) of the pedestrians and of the ring points in the window's frame."""
    loc, vel = np.asarray(scene["loc"], dtype=np.float64), np.asarray(scene["vel"], dtype=np.float64)
    n = len(loc)
    x, y, vx, vy = (f32(a) for a in ((loc[:, 0], loc[:, 1], vel[:, 0], vel[:, 1]) if n else (np.zeros(0),) * 4))
    veh = scene["dynamic_obstacles"]
    M = len(veh)
    cx, cy = f32(veh[k][0])[:2]
    with np.errstate(all="ignore"):
        if not (abs(cx) < NEAR_LIMIT and abs(cy) < NEAR_LIMIT):
            return None
    h = np.asarray(scenarios.vehicle_headings(scene) if headings is None else headings, dtype=np.float32).astype(np.float64)
    hx, hy = h[k]
    vv = f32(np.asarray(scene["dynamic_vel"], dtype=np.float64).reshape(M, 2))
    mx, my = f32(centre)
    c = np.float64(np.float32(cell))
    ox, oy = cx + (hx * mx - hy * my), cy + (hy * mx + hx * my)
    H, m = max(abs(hx), abs(hy), 1.0), abs(mx) + abs(my)
    e_o = U * (max(abs(ox), abs(oy)) + 2.0 * H * m)
    rot = (lambda a, b: (hx * a + hy * b, hx * b - hy * a)) if frame else (lambda a, b: (a, b))
    with np.errstate(all="ignore"):
        alive = (np.abs(x) < NEAR_LIMIT) & (np.abs(y) < NEAR_LIMIT)
    pts = lambda items: np.concatenate([f32(p).reshape(-1, 2) for p in items]) if len(items) else np.zeros((0, 2))
    others = [v for v in range(M) if v != k]
    owner = np.concatenate([np.full(len(veh[v][1]), v, np.int64) for v in others]) if others else np.zeros(0, np.int64)
    kinds = [np.column_stack((x[alive], y[alive])), pts(scene["borders"]), pts([r for _, r in scene["static_obstacles"]]),
             pts([veh[v][1] for v in others])]
    out = []
    with np.errstate(all="ignore"):
        for p in kinds:
            ax, ay = p[:, 0] - ox, p[:, 1] - oy
            A = np.maximum(np.abs(ax), np.abs(ay))
            e_a = U * A + e_o
            e_f = 3.0 * U * H * A + 2.0 * H * e_a if frame else e_a
            margin = 1.01 * (e_f / c + 4.0 * U * H * A / c + U * max(GU, GV) / 2.0)
            fx, fy = rot(ax, ay)
            out.append((fx / c + GU / 2.0, fy / c + GV / 2.0, margin))
        tp = rot(vx[alive] - vv[k, 0], vy[alive] - vv[k, 1])
        tv = rot(vv[owner, 0] - vv[k, 0], vv[owner, 1] - vv[k, 1])
    return out, tp, tv


def classify(pu, pv, margin, GU, GV):
    """Per source: (certain, cell, in_range) -- ``certain``: the float64 coordinates are further than the source's margin from every
    integer on both axes, or clearly out of range; ``cell``: floor's cell id cv * GU + cu, -1 out of range."""
    d = margin
    with np.errstate(all="ignore"):
        near = lambda p, g: (np.abs(p - np.round(p)) <= d) & (p >= -d) & (p <= g + d)
        fin = np.isfinite(pu) & np.isfinite(pv) & np.isfinite(d)
        inside = fin & (pu >= 0) & (pu < GU) & (pv >= 0) & (pv < GV)
        away = ~fin | (pu < -d) | (pu > GU + d) | (pv < -d) | (pv > GV + d)
        certain = away | ~(near(pu, GU) | near(pv, GV))
        cu = np.where(inside, np.floor(np.where(fin, pu, 0.0)), 0).astype(np.int64)
        cv = np.where(inside, np.floor(np.where(fin, pv, 0.0)), 0).astype(np.int64)
    return certain, np.where(inside, cv * GU + cu, -1), inside
