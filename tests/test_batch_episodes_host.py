"""Host-side tests of the batch's episode ends (no GPU): the packer ``batch.episode_arrays`` with every refusal, the host twin
``episode.episode_scene`` on hand-built scenes whose coordinates are exact in fp32 (so every squared distance is known exactly
and the strict ``<`` of each rule can be put on its edge), and the ABI 16 entries in header and binding."""
import os
import re

import numpy as np
import pytest

from carla_social_force_model_amd import _lib
from carla_social_force_model_amd import batch as B_
from carla_social_force_model_amd.batch import episode_arrays
from carla_social_force_model_amd.episode import (EP_AGE, EP_DONE, EP_GOAL_D2, EP_PED_D2, EP_PREV_GOAL_D2, EP_REASON, EP_VEH_D2,
                                                  EP_WALL_D2, REASON_ARRIVED, REASON_NOT_LIVE, REASON_PED_HIT, REASON_TIME_LIMIT,
                                                  REASON_VEH_HIT, episode_scene, radius2)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)
JUST_ABOVE_5 = np.nextafter(np.float32(5), np.float32(6))


def bare(loc, wp=None, **more):
    """A scene dict from planar positions (and waypoints, default the positions + (8, 0)); no geometry unless given."""
    loc = np.asarray(loc, dtype=np.float64).reshape(-1, 2)
    n = len(loc)
    z = np.zeros((n, 1))
    sc = {"loc": np.hstack([loc, z]), "vel": np.zeros((n, 3)),
          "waypoint": np.hstack([loc + [8.0, 0.0] if wp is None else np.asarray(wp, dtype=np.float64).reshape(n, 2), z]),
          "target_speed": np.ones(n)}
    sc.update(more)
    return sc


def ring(center, pts):
    return (np.asarray(center, dtype=np.float64), np.asarray(pts, dtype=np.float64).reshape(-1, 2))


def test_episode_arrays_broadcasts_scalars_and_takes_per_scene_values():
    ag, rg, rp, rv, ms = episode_arrays(3, 0, 1.0, 0.3, [0.0, 0.5, 1e6], 150)
    assert [a.dtype for a in (ag, rg, rp, rv, ms)] == [np.int32, np.float32, np.float32, np.float32, np.int32]
    assert all(a.shape == (3,) and a.flags["C_CONTIGUOUS"] for a in (ag, rg, rp, rv, ms))
    assert ag.tolist() == [0, 0, 0] and ms.tolist() == [150] * 3 and rv.tolist() == [0.0, 0.5, 1e6]
    ag, rg, rp, rv, ms = episode_arrays(2, [-1, 1023], [1], 0, 0.0, [0, 2**31 - 1])
    assert ag.tolist() == [-1, 1023] and rg.tolist() == [1.0, 1.0] and ms.tolist() == [0, 2**31 - 1]
    assert episode_arrays(1, np.int64(4))[0].tolist() == [4]
    # defaults: every test off, no time limit
    ag, rg, rp, rv, ms = episode_arrays(2, 0)
    assert not rg.any() and not rp.any() and not rv.any() and not ms.any()


def test_episode_arrays_refuses_what_the_library_would_refuse():
    for bad in ([0, 1], np.zeros((3, 1), np.int32), np.zeros(4, np.int32)):
        with pytest.raises(ValueError, match="agent: expected a scalar or 3 values"):
            episode_arrays(3, bad)
    for bad in (0.0, "first", None, True):
        with pytest.raises(ValueError, match="agent must be integers"):
            episode_arrays(3, bad)
    for bad in (-2, [0, -2, 0], 1024):
        with pytest.raises(ValueError, match="agent must be -1"):
            episode_arrays(3, bad)
    for name, pos in (("goal_radius", 0), ("ped_radius", 1), ("veh_radius", 2)):
        for bad in (np.nan, -0.5, np.inf, 1.5e6, 1e39, [1.0, np.nan, 1.0]):
            radii = [1.0, 1.0, 1.0]
            radii[pos] = bad
            with pytest.raises(ValueError, match=name + " must be finite, >= 0"):
                episode_arrays(3, 0, *radii)
        radii = [1.0, 1.0, 1.0]
        radii[pos] = [1.0, 2.0]
        with pytest.raises(ValueError, match=name + ": expected a scalar or 3 values"):
            episode_arrays(3, 0, *radii)
        radii[pos] = "wide"
        with pytest.raises(ValueError, match=name + " must be numbers"):
            episode_arrays(3, 0, *radii)
    for bad in (-1, [3, -1, 3], 2**31):
        with pytest.raises(ValueError, match="max_steps must be >= 0"):
            episode_arrays(3, 0, max_steps=bad)
    with pytest.raises(ValueError, match="max_steps must be integers"):
        episode_arrays(3, 0, max_steps=1.5)
    with pytest.raises(ValueError, match="max_steps: expected a scalar or 3 values"):
        episode_arrays(3, 0, max_steps=[1, 2])


def test_radius2_is_the_fp32_radius_squared_in_double_and_rounded_once():
    assert radius2(5.0) == np.float32(25.0) and radius2(0.0) == 0.0
    r = np.float32(0.3)
    assert radius2(0.3) == np.float32(np.float64(r) * np.float64(r))
    assert radius2(JUST_ABOVE_5) > np.float32(25.0)


def test_a_3_4_5_triangle_is_no_hit_at_radius_5_and_one_just_above():
    """Agent at the origin, a pedestrian at (3, 4), a vehicle ring point at (-4, 3): both squared distances are exactly 25."""
    sc = bare([[0, 0], [3, 4], [40, 40]], dynamic_obstacles=[ring([-5, 3], [[-4, 3], [-6, 3], [-6, 5]])])
    rec, (age, prev) = episode_scene(sc, 0, (0.0, 5.0, 5.0), 0)
    assert rec[EP_PED_D2] == 25.0 and rec[EP_VEH_D2] == 25.0 and rec[EP_GOAL_D2] == 64.0
    assert rec[EP_DONE] == 0.0 and rec[EP_REASON] == 0.0 and rec[EP_AGE] == 1.0 and age == 1 and prev == np.float32(64.0)
    rec, _ = episode_scene(sc, 0, (0.0, JUST_ABOVE_5, 5.0), 0)
    assert rec[EP_DONE] == 1.0 and rec[EP_REASON] == REASON_PED_HIT
    rec, _ = episode_scene(sc, 0, (0.0, 5.0, JUST_ABOVE_5), 0)
    assert rec[EP_DONE] == 1.0 and rec[EP_REASON] == REASON_VEH_HIT
    rec, _ = episode_scene(sc, 0, (0.0, JUST_ABOVE_5, JUST_ABOVE_5), 0)
    assert rec[EP_REASON] == REASON_PED_HIT + REASON_VEH_HIT
    # a radius of 0 never fires, even on a coincident pair
    sc = bare([[1, 1], [1, 1]], wp=[[1, 1], [9, 9]], dynamic_obstacles=[ring([1, 1], [[1, 1]])])
    rec, _ = episode_scene(sc, 0, (0.0, 0.0, 0.0), 0)
    assert rec[EP_GOAL_D2] == 0.0 and rec[EP_PED_D2] == 0.0 and rec[EP_VEH_D2] == 0.0 and rec[EP_DONE] == 0.0


def test_a_goal_exactly_at_the_radius_is_not_reached():
    sc = bare([[2, 1]], wp=[[5, 5]])                                    # the goal is 5 m away
    rec, _ = episode_scene(sc, 0, (5.0, 0.0, 0.0), 0)
    assert rec[EP_GOAL_D2] == 25.0 and rec[EP_DONE] == 0.0
    rec, _ = episode_scene(sc, 0, (JUST_ABOVE_5, 0.0, 0.0), 0)
    assert rec[EP_DONE] == 1.0 and rec[EP_REASON] == REASON_ARRIVED


@pytest.mark.parametrize("where", [[2.0e12, 0.0], [0.0, -1.0e12], [np.nan, 0.0], [0.0, np.nan]],
                         ids=["parked-x", "at-the-limit-y", "nan-x", "nan-y"])
def test_an_agent_that_is_not_live_ends_the_episode_and_keeps_prev(where):
    sc = bare([where, [3, 4]], borders=[np.array([[0.0, 1.0], [0.0, 2.0]])])
    rec, (age, prev) = episode_scene(sc, 0, (1.0, 1.0, 1.0), 0, age=4, prev=9.0)
    assert rec[EP_DONE] == 1.0 and rec[EP_REASON] == REASON_NOT_LIVE and rec[EP_AGE] == 5.0
    assert (rec[EP_GOAL_D2:] == INF).all()
    assert age == 5 and prev == np.float32(9.0)                         # the stored value is left alone
    # ... and a parked or NaN row is nobody's pedestrian hit
    rec, _ = episode_scene(sc, 1, (0.0, 1e6, 0.0), 0)
    assert rec[EP_PED_D2] == INF and rec[EP_DONE] == 0.0 and rec[EP_WALL_D2] == 13.0


def test_a_scene_without_an_agent_ends_by_the_time_limit_only():
    sc = bare([[0, 0], [0.1, 0]], wp=[[0, 0], [0, 0]])
    rec, (age, prev) = episode_scene(sc, -1, (5.0, 5.0, 5.0), 2)
    assert rec[EP_DONE] == 0.0 and rec[EP_REASON] == 0.0 and (rec[EP_GOAL_D2:] == INF).all() and np.isnan(prev)
    rec, _ = episode_scene(sc, -1, (5.0, 5.0, 5.0), 2, age=age, prev=prev)
    assert rec[EP_DONE] == 1.0 and rec[EP_REASON] == REASON_TIME_LIMIT and rec[EP_AGE] == 2.0
    rec, _ = episode_scene(bare(np.zeros((0, 2))), -1, (5.0, 5.0, 5.0), 0)           # the empty scene
    assert rec[EP_DONE] == 0.0 and (rec[EP_GOAL_D2:] == INF).all()
    for bad, n in ((0, 0), (2, 2), (-2, 2)):
        with pytest.raises(ValueError, match="is no row"):
            episode_scene(bare(np.zeros((n, 2))), bad, (0, 0, 0), 0)


def test_a_lone_agent_without_geometry_sees_nothing():
    rec, _ = episode_scene(bare([[1, 2]]), 0, (1.0, 1e6, 1e6), 0)
    assert rec[EP_GOAL_D2] == 64.0 and rec[EP_PED_D2] == INF and rec[EP_VEH_D2] == INF and rec[EP_WALL_D2] == INF
    assert rec[EP_DONE] == 0.0


def test_a_vehicle_ring_at_infinity_contributes_infinity():
    away = ring([np.inf, np.inf], np.full((4, 2), np.inf))
    rec, _ = episode_scene(bare([[1, 2]], dynamic_obstacles=[away]), 0, (0.0, 0.0, 1e6), 0)
    assert rec[EP_VEH_D2] == INF and rec[EP_DONE] == 0.0
    rec, _ = episode_scene(bare([[1, 2]], dynamic_obstacles=[away, ring([1, 4], [[1, 4], [2, 4]])]), 0, (0.0, 0.0, 1e6), 0)
    assert rec[EP_VEH_D2] == 4.0 and rec[EP_REASON] == REASON_VEH_HIT


def test_walls_are_borders_and_static_obstacles_and_end_nothing():
    sc = bare([[0, 0]], borders=[np.array([[0.0, 3.0], [0.0, 4.0]]), np.zeros((0, 2))],
              static_obstacles=[ring([2, 0], [[2.0, 0.0], [3.0, 0.0]])])
    rec, _ = episode_scene(sc, 0, (0.0, 1e6, 1e6), 0)
    assert rec[EP_WALL_D2] == 4.0 and rec[EP_DONE] == 0.0
    del sc["static_obstacles"]
    assert episode_scene(sc, 0, (0.0, 0.0, 0.0), 0)[0][EP_WALL_D2] == 9.0


def test_prev_is_the_goal_distance_at_first_and_carried_over_after():
    sc = bare([[0, 0]], wp=[[6, 8]])
    rec, (age, prev) = episode_scene(sc, 0, (1.0, 0.0, 0.0), 0)
    assert rec[EP_GOAL_D2] == 100.0 and rec[EP_PREV_GOAL_D2] == 100.0 and prev == np.float32(100.0) and age == 1
    moved = (np.array([[3.0, 4.0, 0.0]]), np.zeros((1, 3)))
    rec, (age, prev) = episode_scene(sc, 0, (1.0, 0.0, 0.0), 0, age=age, prev=prev, state=moved)
    assert rec[EP_GOAL_D2] == 25.0 and rec[EP_PREV_GOAL_D2] == 100.0 and prev == np.float32(25.0) and age == 2
    rec, _ = episode_scene(sc, 0, (1.0, 0.0, 0.0), 0, age=age, prev=prev, state=moved, waypoints=np.array([[3.0, 4.0, 0.0]]))
    assert rec[EP_GOAL_D2] == 0.0 and rec[EP_PREV_GOAL_D2] == 25.0 and rec[EP_REASON] == REASON_ARRIVED


@pytest.mark.parametrize("max_steps, ends_at", [(0, None), (1, 1), (3, 3)])
def test_the_time_limit(max_steps, ends_at):
    sc = bare([[0, 0]])
    age, prev = 0, np.nan
    for step in range(1, 6):
        rec, (age, prev) = episode_scene(sc, 0, (0.0, 0.0, 0.0), max_steps, age=age, prev=prev)
        over = ends_at is not None and step >= ends_at
        assert rec[EP_AGE] == step and age == step
        assert rec[EP_DONE] == (1.0 if over else 0.0) and rec[EP_REASON] == (REASON_TIME_LIMIT if over else 0)


def test_abi16_entry_points_are_declared():
    assert _lib.ABI_VERSION >= 16
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert int(re.search(r"#define SFM_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    names = ("sfm_batch_set_episodes", "sfm_batch_end_step", "sfm_batch_download_episodes", "sfm_batch_restart_device")
    for name in names:
        assert name in _lib.SYMBOLS and _lib.SINCE[name] == 16
        assert re.search(r"^int " + name + r"\(SfmBatch\* b", header, re.M), name
    assert [len(_lib.SYMBOLS[n][1]) for n in names] == [6, 2, 3, 2]
    for name, val in (("SFM_BATCH_PTR_EPISODES", B_.PTR_EPISODES), ("SFM_BATCH_PTR_DONE", B_.PTR_DONE),
                      ("SFM_BATCH_EPISODE_WIDTH", B_.EPISODE_WIDTH), ("SFM_EPISODE_ARRIVED", B_.REASON_ARRIVED),
                      ("SFM_EPISODE_TIME_LIMIT", B_.REASON_TIME_LIMIT), ("SFM_EPISODE_PED_HIT", B_.REASON_PED_HIT),
                      ("SFM_EPISODE_VEH_HIT", B_.REASON_VEH_HIT), ("SFM_EPISODE_NOT_LIVE", B_.REASON_NOT_LIVE)):
        assert re.search(r"#define " + name + r" " + str(val) + r"\b", header), name
    assert re.search(r"#define SFM_END_STEP_AUTO_RESTART " + str(B_.END_STEP_AUTO_RESTART) + r"u?\b", header)
    assert (B_.EP_DONE, B_.EP_REASON, B_.EP_AGE, B_.EP_GOAL_D2, B_.EP_PREV_GOAL_D2, B_.EP_PED_D2, B_.EP_VEH_D2, B_.EP_WALL_D2) == tuple(range(8))
    assert (EP_DONE, EP_REASON, EP_AGE, EP_GOAL_D2, EP_PREV_GOAL_D2, EP_PED_D2, EP_VEH_D2, EP_WALL_D2) == tuple(range(8))
    lib = _lib.load()                                                   # bound: the built library exports them
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
    for meth in ("set_episodes", "end_step", "episodes", "episode_tensor", "done_tensor", "restart_device"):
        assert callable(getattr(B_.SfmBatch, meth))


def test_device_loop_example_imports_without_a_gpu():
    import importlib.util
    spec = importlib.util.spec_from_file_location("batch_rl_loop_device", os.path.join(ROOT, "examples", "batch_rl_loop_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    assert callable(ex.run) and callable(ex.policy) and ex.N_B == 64
    src = open(os.path.join(ROOT, "examples", "batch_rl_loop_device.py")).read()
    loop = src[src.index("for step in range(steps):"):src.index("last, _ = b.episodes()")]
    assert ".cpu()" not in loop and ".numpy()" not in loop and not re.search(r"\.restart\(|\bage\b", loop)
    assert "end_step(auto_restart=True)" in loop
    # the settings the example passes are ones the packer takes
    episode_arrays(4, 0, ex.GOAL_RADIUS, ex.PED_RADIUS, ex.VEH_RADIUS, 150)
