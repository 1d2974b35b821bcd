"""The crowd the restart-noise tests share (tests/test_batch_reset_host.py, tests/test_batch_reset_gpu.py): six scenes of
1, 2, 63, 65, 300 and 1 024 rows -- a lone row, the wave boundary, the pass boundary at the workgroup's 256 lanes and the limit -- with
their noise settings, and the twin's answer for a restart.  Built once; nothing changes it.  Pure NumPy.

Scene 0 (1 row): geometry, a movable row.  Scene 1 (2 rows): no geometry at all.  Scene 2 (63 rows): geometry, every box zero (all
rows fixed, goals stay bit for bit but for a -0 goal).  Scenes 3 .. 5 (65, 300, 1 024 rows): dense enough to reject -- a jittered grid
2 m apart, boxes of 1 m, min_gap 0.6 m, point_gap 0.3 m -- with designed rows in scene 3: row 0 is fixed (box 0) and row 1 stands 0.2 m from
it inside a box of 0.05 m, so it can never be placed (a fallback); and in scene 4 two rows that are not live (parked far away).
Every scene with geometry has 3 borders, 2 static obstacles and 2 device-side vehicles; vehicle 0 is tracked and has a delay."""
from functools import lru_cache

import numpy as np

from carla_social_force_model_amd import reset, scenarios

SIZES = (1, 2, 63, 65, 300, 1024)
DTS = (0.05, 0.04, 0.05, 0.03, 0.05, 0.05)
SEEDS = (101, 202, 303, 404, 505, 606)
MIN_GAP, POINT_GAP, TRIES = 0.6, 0.3, 8
DELAY = 6                      # vehicle 0 of a scene: up to 6 ticks late (vehicle 1 runs free: its delay is ignored)
TICKS = 24                     # the length the tracks are planned for
BARE, ZERO_BOXES, DESIGNED, GHOSTS = 1, 2, 3, 4      # the scenes with a special role
FAR = 3.0e15


@lru_cache(maxsize=None)
def scenes():
    out = []
    for k, n in enumerate(SIZES):
        geo = k != BARE
        sc = vars(scenarios.make_scenario(n, 9100 + k, n_borders=3 if geo else 0, n_static=2 if geo else 0, n_dynamic=2 if geo else 0,
                                          border_len=(5.0, 12.0)))
        if k == DESIGNED:
            sc["loc"][1, :2] = scenarios._f32(sc["loc"][0, :2] + np.array([0.2, 0.0]))
        if k == GHOSTS:
            sc["loc"][7, 0], sc["loc"][200, 0] = np.float32(FAR), np.float32(FAR + 2.0e12)
            sc["vel"][[7, 200]] = 0.0
        out.append(sc)
    return out


@lru_cache(maxsize=None)
def tracks():
    """Per scene None, or [vehicle 0's track, None]."""
    return [[scenarios.make_track_plan(sc, 9200 + k, TICKS, dt=DTS[k])[0], None] if sc["dynamic_obstacles"] else None
            for k, sc in enumerate(scenes())]


@lru_cache(maxsize=None)
def boxes():
    """(pos_box, goal_box): per scene (N_b, 2) float64."""
    pos, goal = [], []
    for k, n in enumerate(SIZES):
        p, g = np.full((n, 2), 1.0), np.full((n, 2), 2.5)
        p[:, 1] = 0.75
        if k == ZERO_BOXES:
            p[:], g[:] = 0.0, 0.0
        if k == DESIGNED:
            p[0], p[1] = 0.0, 0.05
        pos.append(p)
        goal.append(g)
    return pos, goal


def delays():
    """track_delay over the concatenated vehicles (2 per scene with geometry)."""
    return np.concatenate([np.array([DELAY, 3], dtype=np.int32) if sc["dynamic_obstacles"] else np.zeros(0, np.int32) for sc in scenes()])


def noise_args():
    """What SfmBatch.set_restart_noise takes for the whole batch."""
    pos, goal = boxes()
    return dict(seeds=np.array(SEEDS, dtype=np.uint32), pos_box=pos, goal_box=goal, min_gap=MIN_GAP, point_gap=POINT_GAP, tries=TRIES,
                track_delay=delays())


def twin(k, e, state=None, vehicles=None, waypoints=None, shift=0, tau=0, seed=None, detail=False):
    """Scene k's restart e as the twin computes it; the restored first ticks are the plan's, moved by ``shift``."""
    sc = scenes()[k]
    tr = tracks()[k]
    if tr is not None:
        tr = [None if t is None else dict(t, first_tick=t["first_tick"] + shift) for t in tr]
    pos, goal = boxes()
    return reset.resample_scene(sc, SEEDS[k] if seed is None else seed, e, pos[k], goal[k], MIN_GAP, POINT_GAP, TRIES, state=state,
                                vehicles=vehicles, waypoints=waypoints, tracks=tr,
                                track_delay=np.array([DELAY, 3]) if tr is not None else None, tau=tau, detail=detail)
