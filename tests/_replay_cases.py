"""Shared cases of the observed-track tests (tests/test_batch_replay_host.py, tests/test_batch_replay_gpu.py): scene and track
builders whose coordinates are all fp32-representable, a driver that runs the twin frame by frame, and the bound on where a replayed
row lies after its ticks.

Where a replayed row lies after ``every`` ticks
-----------------------------------------------
A row observed at f and f + 1, at o and o1 (fp32), is placed at x_0 = o exactly with the velocity of the rules (include/sfm_hip.h),
per component, with u = 2^-24 the unit roundoff of fp32, D = o1 - o the exact difference and h = every * dt the exact product of
the integer and the fp32 step length:

    d   = fl(o1 - o)        = D (1 + e1)                  |e1| <= u
    inv = fl(1 / h)         = (1 / h) (1 + e2)            |e2| <= u     (formed in double, rounded once)
    v   = fl(d * inv)       = (D / h) (1 + e1)(1 + e2)(1 + e3)          |e3| <= u

so ``every`` exact steps of dt * v would end at o + D (1 + e1)(1 + e2)(1 + e3): off o1 by at most |D| (3u + 3u^2 + u^3).  Each tick
is one fma, x_{k+1} = fl(dt v + x_k) = (dt v + x_k)(1 + g_k), |g_k| <= u: it adds an error of at most u |x_{k+1}|, and every
x_k lies between o and o1 up to the errors already counted, so |x_k| <= M = max(|o|, |o1|) to first order.  The errors of earlier
ticks are carried along unchanged (the later steps add the same dt v to a shifted x).  In all

    |x_every - o1| <= u (3 |D| + every M) + O(u^2)

``arrival_bound`` returns u (3.01 |D| + 1.01 every M): the slack of one percent covers the second-order terms (u ~ 6e-8).  It is
derived from the roundings alone; nothing in it was measured.
"""
import numpy as np

from carla_social_force_model_amd import replay, scenarios
from carla_social_force_model_amd.config import default_sfm_config

U = 2.0 ** -24
DT = 0.05
f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)      # a float64 array of fp32-representable values

SIZES = (0, 1, 3, 65, 257, 1024)         # an empty scene, a lone row, the wave boundary, the 256-lane stride, the cap
FRAMES = (0, 6, 3, 6, 5, 4)              # scenes of different lengths share the batch
RUN_FRAMES = 7                           # every scene is also run beyond its last frame
EVERY = (1, 3)


def arrival_bound(o, o1, every):
    o, o1 = np.asarray(o, dtype=np.float64), np.asarray(o1, dtype=np.float64)
    return U * (3.01 * np.abs(o1 - o) + 1.01 * every * np.maximum(np.abs(o), np.abs(o1)))


def config():
    return default_sfm_config(scenarios.ALL_FORCES)


def crowd(n, seed, geo=True, dynamic=0):
    sc = vars(scenarios.make_scenario(n, seed, n_borders=6 if geo else 0, n_static=3 if geo else 0, n_dynamic=dynamic,
                                      border_len=(3.0, 15.0)))
    sc["radius"] = f32(np.random.default_rng(seed + 17).uniform(0.2, 0.45, n))
    for k in ("loc", "vel", "waypoint"):
        sc[k] = f32(sc[k])
    return sc


def tracks_for(sc, F, every, seed, dt=DT):
    """A recording of F frames for a scene: every row walks from its uploaded position with a velocity of its own; who is seen when
    follows the row index, so that every class occurs in every scene that is large enough.  Returns (obs (F, n, 2) float32, roles
    (n,) uint8, v0 (n, 2) float32).  By index i:
        i % 7 == 3    role 0 (not part of the data; its track is all NaN)
        i % 11 == 5   role 2 (scored), else role 1 (replayed)
        i % 13 == 0 and i > 0   never observed
        i % 5 == 1    a late arrival (first seen at frame 1 + i % 2)
        i % 5 == 2    an early leaver (last seen at frame F - 2)
        i % 5 == 3    a gap at frame 2
        i % 4 == 1    an initial velocity is given"""
    n = len(sc["loc"])
    rng = np.random.default_rng(seed)
    h = every * dt
    vel = f32(rng.uniform(-1.5, 1.5, (n, 2)))
    obs = np.full((F, n, 2), np.nan, np.float32)
    i = np.arange(n)
    for f in range(F):
        obs[f] = np.float32(sc["loc"][:, :2] + f * h * vel)
    roles = np.where(i % 7 == 3, 0, np.where(i % 11 == 5, 2, 1)).astype(np.uint8)
    for f in range(F):
        gone = (roles == 0) | ((i % 13 == 0) & (i > 0))
        gone |= (i % 5 == 1) & (f < 1 + i % 2)
        gone |= (i % 5 == 2) & (f > F - 2)
        gone |= (i % 5 == 3) & (f == 2)
        obs[f, gone] = np.nan
    v0 = np.full((n, 2), np.nan, np.float32)
    v0[i % 4 == 1] = np.float32(rng.uniform(-1.0, 1.0, (int((i % 4 == 1).sum()), 2)))
    return obs, roles, v0


def mixed_batch(every):
    """(scenes, tracks, roles, v0) of the device tests: scenes of 0, 1, 3, 65, 257 and 1 024 rows with 0 .. 6 frames; all five
    forces everywhere; borders, static obstacles and vehicles (which move on the device) in the scenes of 65 and 257 rows."""
    scenes = [crowd(n, 7300 + q, geo=q in (3, 4), dynamic=3 if q in (3, 4) else 0) for q, n in enumerate(SIZES)]
    packs = [tracks_for(sc, F, every, 7400 + q) for q, (sc, F) in enumerate(zip(scenes, FRAMES))]
    return scenes, [p[0] for p in packs], [p[1] for p in packs], [p[2] for p in packs]


def classes(tracks, roles):
    """How many rows of each class a batch holds: late arrivals, early leavers, gaps inside a span, never observed, each for the
    replayed and the scored rows, and the rows of role 0."""
    out = {"role0": 0}
    for name in ("late", "early", "gap", "never"):
        out[name + "1"] = out[name + "2"] = 0
    for obs, r in zip(tracks, roles):
        F, n = obs.shape[0], obs.shape[1]
        out["role0"] += int((r == 0).sum())
        if F == 0:
            continue
        seen = ~np.isnan(obs[..., 0])
        f0, f1 = replay.spans(obs)
        ever = f0 <= f1
        inside = np.array([ever[i] and (~seen[f0[i]:f1[i] + 1, i]).any() for i in range(n)], dtype=bool)
        for role in (1, 2):
            m = r == role
            out[f"late{role}"] += int((m & ever & (f0 > 0)).sum())
            out[f"early{role}"] += int((m & ever & (f1 < F - 1)).sum())
            out[f"gap{role}"] += int((m & inside).sum())
            out[f"never{role}"] += int((m & ~ever).sum())
    return out


def frame_rates(B, every, dt=DT):
    return [replay.frame_rate(every, np.float32(dt))] * B


def stage(scenes):
    """The uploaded state of every scene as the frame kernel finds it: a list of ``replay.new_scene`` dicts."""
    return [replay.new_scene(np.hstack([np.float32(sc["loc"])[:, :2], np.float32(sc["vel"])[:, :2]]).reshape(-1, 4)) for sc in scenes]


# ---- the sweep's scene: one scored row walking into three replayed rows ----------------------------------------------------------
SWEEP_FRAMES = 6
SWEEP_EVERY = 2
SWEEP_A = (1.0, 0.5, 2.0, 4.0)           # the pedestrian force's A as multiples of the truth: the truth comes first


def sweep_scene():
    """(scene, obs, roles, v0): row 0 is scored, walking along +x with v0 = (1.25, 0) into rows 1 .. 3, who are replayed, cross its
    path within 3 m of it and are observed in every frame.  Row 0 is observed at its first and last frame only."""
    loc = f32([[0.0, 0.0], [2.0, 0.5], [2.5, -0.75], [1.5, 1.25]])
    vel = f32([[1.25, 0.0], [-0.5, -0.25], [-0.25, 0.5], [0.0, -0.75]])
    n = 4
    z = np.zeros((n, 1))
    sc = {"loc": np.hstack([loc, z]), "vel": np.hstack([vel, z]), "waypoint": np.hstack([f32([[8.0, 0.0]] * n), z]),
          "target_speed": np.full(n, 1.25), "radius": np.full(n, 0.25)}
    h = SWEEP_EVERY * DT
    obs = np.stack([np.float32(loc + f * h * vel) for f in range(SWEEP_FRAMES)])
    obs[1:SWEEP_FRAMES - 1, 0] = np.nan
    roles = np.array([2, 1, 1, 1], np.uint8)
    v0 = np.full((n, 2), np.nan, np.float32)
    v0[0] = (1.25, 0.0)
    return sc, obs, roles, v0


def sweep_config(a_factor):
    cfg = default_sfm_config(("acceleration_force", "pedestrian_force"))
    cfg["pedestrian_force"]["A"] = float(np.float32(cfg["pedestrian_force"]["A"] * a_factor))
    return cfg
