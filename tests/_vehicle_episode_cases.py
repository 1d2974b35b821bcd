"""The scenes the vehicle-episode tests share (tests/test_batch_vehicle_episodes_host.py, tests/test_batch_vehicle_episodes_gpu.py):
one mixed batch, so that one upload serves many tests.  Built once; nothing changes it.  Pure NumPy.

    scene  rows  vehicles  agents          geometry                what it is for
      0       0      1     0               -                       no pedestrian: ped_gap2 = +inf
      1       1      1     0               -                       one lane of the row loop
      2      65      2     0               2 borders, 1 static     one row past a lane stride; a vehicle that is no agent
      3      64      5     all             2 borders, 1 static     a wave takes a second vehicle (4 waves, 5 agents)
      4    1024      9     all             2 borders, 1 static     the largest scene; a wave takes up to three vehicles
      5       3     70     0, 63, 64, 69   -                       many rings: the own ring's range begins / ends anywhere
      6       5      0     -               1 border                no vehicles
      7      10      2     none            1 border                vehicles, none an agent: the scene is never written
      8       4      2     0 (tracked, absent)                     an agent that is not live
      9       4      2     1, heading exactly (0, 1); vehicle 0 tracked, absent: its ring lies at +inf, inf * 0 = NaN
     10       2      1     0               3 borders  (> 256 points)
     11       2      1     0               8 static   (> 256 points)
     12       2      1     0               3 borders, 8 static

Vehicles stand inside the crowd, near a border or a static obstacle where the scene has one, so that every reason fires.

The bound of the host test is derived here.  u = 2^-24 is the unit roundoff of fp32; every fmaf is one rounding.  For a candidate p
and a box (c, h, e) write d = p - c (exact, from the fp32 inputs), R = |d|, and let (ut, vt) be d's coordinates along the UNIT vectors
h / |h| and its left normal -- the float64 statement is the distance from (ut, vt) to the rectangle |ut| <= ex, |vt| <= ey.
  1. dx_f = dx (1 + e1), dy_f = dy (1 + e2); t = fl(hy dy_f) = hy dy_f (1 + e3); u_f = fmaf(hx, dx_f, t) = (hx dx_f + t)(1 + e4).
     So |u_f - (hx dx + hy dy)| <= (|hx dx| + |hy dy|) E3 <= |h| R E3 with E3 = (1 + u)^3 - 1 (Cauchy-Schwarz); v_f likewise.
  2. The stored heading is not exactly unit: | |h|^2 - 1 | <= H2 = 6u + 64u^2 for a driven heading (tests/_driving_cases.py), less
     for the fp32 cos / sin of a yaw.  hx dx + hy dy = |h| ut, so it is off ut by at most DH |ut| <= DH R, DH = H2 / 2 + H2^2 / 8
     (sqrt(1 + x) - 1 lies within x / 2 -+ x^2 / 8).  Together |u_f - ut| <= EU R, EU = E3 (1 + DH) + DH.
  3. w = |u_f| - ex; ax_f = fmaxf(fl(w), 0) = max(w, 0)(1 + e5) (a rounding keeps the sign).  max(., 0) is 1-Lipschitz, so
     |max(w, 0) - ax| <= EU R, and max(w, 0) <= ax + EU R <= R (1 + EU): |ax_f - ax| <= EA R, EA = EU + u (1 + EU).  ay likewise.
  4. gap2_f = fmaf(ax_f, ax_f, fl(ay_f ay_f)) = (ax_f^2 + ay_f^2 (1 + e6))(1 + e7).  |ax_f^2 - ax^2| <= EA R (2 ax + EA R); summed
     over both axes with ax + ay <= sqrt(2) gap <= sqrt(2) R: |S_f - gap^2| <= ES R^2, ES = EA (2 sqrt(2) + 2 EA); the two roundings
     add (2u + u^2) S_f <= (2u + u^2)(1 + ES) R^2.
  => |gap2_f - gap2_64| <= GAP2_REL * R^2,   GAP2_REL = ES + (2u + u^2)(1 + ES)   (about 22 u).
A slot is a minimum.  With i the float64 minimiser and j the fp32 one, min_f <= f_i <= t_i + eps_i and min_f = f_j >= t_j - eps_j >=
min_t - eps_j: |min_f - min_t| <= GAP2_REL * max(R_i, R_j)^2 -- the bound of the test, with no case left out (a tie changes which
index is taken, not the value)."""
from functools import lru_cache

import numpy as np

from carla_social_force_model_amd import episode, scenarios

U = 2.0 ** -24
H2 = 6.0 * U + 64.0 * U * U
DH = H2 / 2.0 + H2 * H2 / 8.0
E3 = (1.0 + U) ** 3 - 1.0
EU = E3 * (1.0 + DH) + DH
EA = EU + U * (1.0 + EU)
ES = EA * (2.0 * np.sqrt(2.0) + 2.0 * EA)
GAP2_REL = ES + (2.0 * U + U * U) * (1.0 + ES)

SIZES = (0, 1, 65, 64, 1024, 3, 5, 10, 4, 4, 2, 2, 2)
VEHICLES = (1, 1, 2, 5, 9, 70, 0, 2, 2, 2, 1, 1, 1)
GEO = {2: (2, 1), 3: (2, 1), 4: (2, 1), 6: (1, 0), 7: (1, 0), 10: (3, 0), 11: (0, 8), 12: (3, 8)}     # borders, static
B = len(SIZES)
DTS = (0.05, 0.05, 0.04, 0.05, 0.03, 0.05, 0.05, 0.04, 0.05, 0.05, 0.05, 0.03, 0.05)
AGENTS = {0: (0,), 1: (0,), 2: (0,), 3: (0, 1, 2, 3, 4), 4: tuple(range(9)), 5: (0, 63, 64, 69), 8: (0,), 9: (1,), 10: (0,), 11: (0,), 12: (0,)}
ABSENT = {8: 0, 9: 0}            # scene: its tracked vehicle, absent for the whole test (its track starts at tick 1000)
UP_SCENE, UP_VEHICLE = 9, 1      # the agent whose heading is exactly (0, 1)
WALL_SCENES = (10, 11, 12)
EXTENT = (2.4, 1.0)
# the scenes' radii and time limits: contacts and arrivals happen, the time limit fires within three evaluations
GOAL_R = (3.0, 0.0, 3.0, 6.0, 6.0, 3.0, 1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0)
PED_R = (1.0, 0.5, 0.5, 0.5, 0.3, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0, 0.5)
VEH_R = (1.0, 1.0, 0.5, 0.5, 0.5, 0.3, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0)
WALL_R = (1.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.6, 0.6, 0.6)
MAX_STEPS = (0, 2, 0, 3, 0, 0, 1, 1, 0, 3, 0, 2, 0)


def _place(c, heading):
    return scenarios.place_ring_heading_f32(c, heading, scenarios.ring_local_offsets(*EXTENT))


@lru_cache(maxsize=None)
def scenes():
    """The scene dicts.  ``dynamic_heading`` holds the fp32 headings the device is given (``boxes()``), and the rings are placed from
    them, so that a heading can be exactly (0, 1)."""
    out = []
    for k, (n, m) in enumerate(zip(SIZES, VEHICLES)):
        nb, ns = GEO.get(k, (0, 0))
        sc = vars(scenarios.make_scenario(n, 9100 + k, n_borders=nb, n_static=ns, n_dynamic=m, border_len=(14.0, 30.0)))
        rng = np.random.default_rng(9200 + k)
        side = max(float(sc["world_side"]), 8.0)
        yaw = np.asarray(sc["dynamic_yaw"], dtype=np.float64)
        h = np.column_stack((np.cos(yaw), np.sin(yaw))).astype(np.float32)
        cs = []
        for v in range(m):
            if k in WALL_SCENES or (nb + ns and v == 0):               # beside a wall point
                walls = list(sc["borders"]) + [r for _, r in sc["static_obstacles"]]
                w = walls[v % len(walls)]
                c = w[len(w) // 3] + rng.uniform(-1.2, 1.2, 2)
            elif n and v % 2 == 0:                                     # beside a pedestrian
                c = sc["loc"][rng.integers(0, n), :2] + rng.uniform(-1.5, 1.5, 2)
            elif cs:                                                   # beside another vehicle
                c = cs[rng.integers(0, len(cs))] + rng.uniform(-4.0, 4.0, 2)
            else:
                c = rng.uniform(0.0, side, 2)
            cs.append(np.float32(c).astype(np.float64))
        if k == UP_SCENE:
            h[UP_VEHICLE] = (0.0, 1.0)
        sc["dynamic_vel"] = np.float32(sc["dynamic_vel"] * 0.1).astype(np.float64)
        sc["dynamic_heading"] = h
        sc["dynamic_obstacles"] = [(cs[v], _place(cs[v], h[v])) for v in range(m)]
        sc["dynamic_extent"] = np.tile(np.array(EXTENT), (m, 1))
        out.append(sc)
    for k in WALL_SCENES:
        pts = sum(len(p) for p in out[k]["borders"]) + sum(len(r) for _, r in out[k]["static_obstacles"])
        assert pts > 256, (k, pts)
    return out


def boxes(which=None):
    """What SfmBatch.set_dynamic_boxes takes (the tuple of ``batch.pack_boxes``) with the headings of ``scenes()``."""
    from carla_social_force_model_amd.batch import pack_boxes
    which = range(B) if which is None else which
    t = list(pack_boxes([scenes()[k] for k in which]))
    h = [scenes()[k]["dynamic_heading"] for k in which if VEHICLES[k]]
    h = np.concatenate(h) if h else np.zeros((0, 2), np.float32)
    t[6], t[7] = np.ascontiguousarray(h[:, 0], dtype=np.float32), np.ascontiguousarray(h[:, 1], dtype=np.float32)
    return tuple(t)


def tracks(which=None):
    """What SfmBatch.set_vehicle_tracks takes: the vehicles of ``ABSENT`` are tracked and enter at tick 1000."""
    which = range(B) if which is None else which
    out = []
    for k in which:
        if k not in ABSENT:
            out.append(None)
            continue
        per = [None] * VEHICLES[k]
        per[ABSENT[k]] = {"xy": np.array([[1.0, 1.0], [1.5, 1.0]]), "yaw": np.zeros(2), "speed": np.ones(2), "first_tick": 1000}
        out.append(per)
    return out


@lru_cache(maxsize=None)
def agents():
    """Per scene (M_b,) bool."""
    out = []
    for k, m in enumerate(VEHICLES):
        a = np.zeros(m, bool)
        a[list(AGENTS.get(k, ()))] = True
        out.append(a)
    return out


@lru_cache(maxsize=None)
def goals():
    """Per scene (M_b, 2): a few metres ahead of each vehicle, so that some arrive."""
    out = []
    for k, sc in enumerate(scenes()):
        rng = np.random.default_rng(9300 + k)
        c = np.array([c for c, _ in sc["dynamic_obstacles"]]).reshape(-1, 2)
        out.append(np.float32(c + rng.uniform(-6.0, 6.0, c.shape)).astype(np.float64))
    return out


def extents(which=None):
    which = range(B) if which is None else which
    return [np.tile(np.array(EXTENT), (VEHICLES[k], 1)) for k in which]


def episode_args(which=None):
    """What SfmBatch.set_vehicle_episodes takes, for the whole batch or the scenes ``which``."""
    which = list(range(B) if which is None else which)
    pick = lambda t: [t[k] for k in which]
    return dict(agents=[agents()[k] for k in which], goals=[goals()[k] for k in which], extents=extents(which), goal_radius=pick(GOAL_R),
                ped_radius=pick(PED_R), veh_radius=pick(VEH_R), wall_radius=pick(WALL_R), max_steps=pick(MAX_STEPS))


def absent_scene(k):
    """Scene k as the device holds it with the tracks set: the vehicles of ``ABSENT`` at +inf (``scenarios.place_tracked``)."""
    sc = dict(scenes()[k])
    if k in ABSENT:
        veh = list(sc["dynamic_obstacles"])
        v = ABSENT[k]
        veh[v] = (np.full(2, np.inf), np.full_like(veh[v][1], np.inf))
        sc["dynamic_obstacles"] = veh
    return sc


def twin(k, state=None, vehicles=None, headings=None, ages=None, prevs=None, agent_flags=None):
    """Scene k's evaluation as the twin computes it."""
    sc = absent_scene(k)
    return episode.vehicle_episode_scene(sc, agents()[k] if agent_flags is None else agent_flags, goals()[k], extents((k,))[0],
                                         (GOAL_R[k], PED_R[k], VEH_R[k], WALL_R[k]), MAX_STEPS[k], ages=ages, prevs=prevs, state=state,
                                         vehicles=vehicles, headings=sc["dynamic_heading"] if headings is None else headings)


def rect_gap2_64(centre, heading, extent, pts):
    """The float64 statement: per point (P,) the squared distance to the rectangle of half-extents ``extent`` around ``centre`` whose
    axes are the UNIT vector along ``heading`` and its left normal, and R^2 = |p - c|^2; points that are not live: +inf."""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    c, h, e = (np.asarray(a, dtype=np.float64) for a in (centre, heading, extent))
    h = h / np.hypot(h[0], h[1])
    ok = (np.abs(p[:, 0]) < 1.0e12) & (np.abs(p[:, 1]) < 1.0e12)
    gap, r2 = np.full(p.shape[0], np.inf), np.full(p.shape[0], np.inf)
    d = p[ok] - c
    ut, vt = d @ h, d @ np.array([-h[1], h[0]])
    ax, ay = np.maximum(np.abs(ut) - e[0], 0.0), np.maximum(np.abs(vt) - e[1], 0.0)
    gap[ok], r2[ok] = ax * ax + ay * ay, (d * d).sum(axis=1)
    return gap, r2
