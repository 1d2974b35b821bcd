"""Host-side tests of the batch's vehicle tracks (no GPU): the packer (CSR layout, float32 roundings, refusals), the VehicleSpawner
mirror and ``tracks_from_spawners`` against keyframes and ticks written out by hand from the reference's lines
(vehicle_spawner.py:164, :197-198, :140-143, :183-185; run_simulation.py:52-67), the host twin ``place_tracked`` at the boundaries
of a track, the synthetic recipe, and the ABI 12 entries in header and binding."""
import os
import re

import numpy as np
import pytest

from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import MAX_TRACK_KEYS, pack_tracks
from carla_social_force_model_amd.spawner import PedSpawner, birth_ticks
from carla_social_force_model_amd.spawner import release_times as ped_release_times
from carla_social_force_model_amd.vehicle_spawner import VehicleSpawner, first_ticks, release_times, tracks_from_spawners
from oracle import sfm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _track(L, first, seed=0):
    rng = np.random.default_rng(seed)
    return {"xy": rng.uniform(-20.0, 20.0, (L, 2)), "yaw": rng.uniform(-4.0, 4.0, L), "speed": rng.uniform(0.0, 1.4, L),
            "first_tick": first}


def _scene(M, ext=(2.4, 1.0), n=4):
    sc = vars(scenarios.make_scenario(n, 5, n_dynamic=M))
    sc["dynamic_extent"] = np.tile(np.asarray(ext, dtype=np.float64), (M, 1))
    return sc


# ---- pack_tracks ----------------------------------------------------------------------------------------------------------------
def test_pack_tracks_layout_and_roundings():
    scenes = [_scene(2), _scene(0), _scene(3)]
    t0, t1, t2 = _track(3, -3, 1), _track(1, 0, 2), _track(5, 7, 3)
    pt = pack_tracks([[t0, None], None, [None, t1, t2]], scenes)
    assert pt["trk_off"].dtype == np.int32 and pt["first_tick"].dtype == np.int32
    assert pt["trk_off"].tolist() == [0, 3, 3, 3, 4, 9]
    assert pt["first_tick"].tolist() == [-3, 0, 0, 0, 7]
    for key in ("kx", "ky", "kvx", "kvy", "kcos", "ksin"):
        assert pt[key].dtype == np.float32 and pt[key].shape == (9,)
    for tr, lo in ((t0, 0), (t1, 3), (t2, 4)):
        L = len(tr["yaw"])
        sl = slice(lo, lo + L)
        assert np.array_equal(pt["kx"][sl], tr["xy"][:, 0].astype(np.float32))
        assert np.array_equal(pt["ky"][sl], tr["xy"][:, 1].astype(np.float32))
        # velocity: the float64 product, rounded once -- NOT the product of the rounded factors
        assert np.array_equal(pt["kvx"][sl], (tr["speed"] * np.cos(tr["yaw"])).astype(np.float32))
        assert np.array_equal(pt["kvy"][sl], (tr["speed"] * np.sin(tr["yaw"])).astype(np.float32))
        # cos / sin: rounded as place_ring_f32 rounds them
        assert np.array_equal(pt["kcos"][sl], np.array([np.float32(np.cos(y)) for y in tr["yaw"]]))
        assert np.array_equal(pt["ksin"][sl], np.array([np.float32(np.sin(y)) for y in tr["yaw"]]))
    # the vehicles' scene_item_off says the same as the scenes
    pt2 = pack_tracks([[t0, None], None, [None, t1, t2]], np.array([0, 2, 2, 5], dtype=np.int32))
    assert all(np.array_equal(pt[k], pt2[k]) for k in pt)


def test_pack_tracks_velocity_is_rounded_once():
    """A speed and yaw for which rounding the factors first gives another float32 than rounding the float64 product."""
    rng = np.random.default_rng(11)
    yaw, sp = rng.uniform(-3.0, 3.0, 4000), rng.uniform(0.1, 1.4, 4000)
    once = (sp * np.cos(yaw)).astype(np.float32)
    twice = sp.astype(np.float32) * np.cos(yaw).astype(np.float32)
    k = int(np.nonzero(once != twice)[0][0])
    pt = pack_tracks([[{"xy": np.zeros((1, 2)), "yaw": yaw[k:k + 1], "speed": sp[k:k + 1], "first_tick": 0}]], [_scene(1)])
    assert pt["kvx"][0] == once[k] and pt["kvx"][0] != twice[k]


def test_pack_tracks_without_any_track():
    pt = pack_tracks([None, [None, None]], [_scene(0), _scene(2)])
    assert pt["trk_off"].tolist() == [0, 0, 0] and pt["first_tick"].tolist() == [0, 0] and pt["kx"].shape == (0,)


@pytest.mark.parametrize("bad, match", [
    (lambda t: t.pop("yaw"), "no yaw"),
    (lambda t: t.update(xy=np.zeros((3, 3))), r"xy must be \(L,2\)"),
    (lambda t: t.update(xy=np.zeros((0, 2)), yaw=np.zeros(0), speed=np.zeros(0)), "at least one keyframe"),
    (lambda t: t.update(yaw=np.zeros(2)), "3 keyframes need 3"),
    (lambda t: t.update(speed=np.zeros(4)), "3 keyframes need 3"),
    (lambda t: t.update(first_tick=1.5), "first_tick must be an integer"),
    (lambda t: t.update(first_tick=2 ** 31), "first_tick must be an integer"),
    (lambda t: t["xy"].__setitem__((1, 0), np.nan), "finite"),
    (lambda t: t["yaw"].__setitem__(0, np.inf), "finite"),
    (lambda t: t["speed"].__setitem__(2, 1e39), "finite"),
])
def test_pack_tracks_refuses(bad, match):
    t = _track(3, 0)
    bad(t)
    with pytest.raises(ValueError, match=match) as e:
        pack_tracks([[None, t]], [_scene(2)])
    assert "scene 0, vehicle 1" in str(e.value)


def test_pack_tracks_refuses_counts_and_types():
    with pytest.raises(ValueError, match="2 track lists for 1 scenes"):
        pack_tracks([None, None], [_scene(1)])
    with pytest.raises(ValueError, match="scene 0: 1 tracks for 2 vehicles"):
        pack_tracks([[None]], [_scene(2)])
    with pytest.raises(ValueError, match="must be a dict or None"):
        pack_tracks([[3]], [_scene(1)])
    with pytest.raises(ValueError, match="scene_item_off"):
        pack_tracks([None], np.array([1, 2]))


def test_pack_tracks_refuses_more_keyframes_than_the_cap():
    L = MAX_TRACK_KEYS // 2 + 1
    t = {"xy": np.zeros((L, 2)), "yaw": np.zeros(L), "speed": np.zeros(L), "first_tick": 0}
    with pytest.raises(ValueError, match=f"more than the {MAX_TRACK_KEYS}"):
        pack_tracks([[t, t]], np.array([0, 2]))


# ---- the VehicleSpawner mirror and tracks_from_spawners -------------------------------------------------------------------------
def _lists(L, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-30.0, 30.0, (L, 2)), rng.uniform(-3.0, 3.0, L), rng.uniform(0.0, 10.0, L)


@pytest.mark.parametrize("L", [2, 3, 40])
def test_keyframes_are_entries_1_to_L_minus_1(L):
    """vehicle_spawner.py:197-198 pops entry 0 of trajectory / headings for the spawn transform, :164 keeps speeds[1:]; the release
    tick already teleports to the next entry (run_simulation.py:58-62): L entries -> the L - 1 keyframes 1 .. L-1."""
    traj, head, speeds = _lists(L, L)
    sp = VehicleSpawner(traj.tolist(), head.tolist(), speeds.tolist(), quantity=1, spawn_time=0.0, spawn_interval=5.0)
    assert np.array_equal(sp.spawn_location, traj[0]) and sp.spawn_heading == head[0]
    assert len(sp.trajectory) == len(sp.headings) == len(sp.speeds) == L - 1
    (tr,) = tracks_from_spawners([sp], 0.05, 0.0)
    assert np.array_equal(tr["xy"], traj[1:]) and np.array_equal(tr["yaw"], head[1:]) and np.array_equal(tr["speed"], speeds[1:])
    assert tr["first_tick"] == 0
    # seen in ticks 0 .. L-2, gone in tick L-1: the tick in which the reference finds its list empty (run_simulation.py:63-66)
    assert [scenarios.track_present(tr, t) for t in (-1, 0, L - 2, L - 1)] == [False, True, True, False]
    assert sp.quantity == 1 and sp.next_spawn_time == 0.0                       # the spawner is not advanced


def test_ready_to_spawn_is_the_references():
    """vehicle_spawner.py:183-185: due while next_spawn_time <= sim_time, each True adds one interval (float64 +=)."""
    sp = VehicleSpawner(*_lists(3, 1), quantity=3, spawn_time=0.3, spawn_interval=0.07)
    assert not sp.ready_to_spawn(0.29)
    assert sp.ready_to_spawn(0.3) and sp.next_spawn_time == 0.3 + 0.07
    assert not sp.ready_to_spawn(0.3)
    assert sp.ready_to_spawn(1.0) and sp.next_spawn_time == (0.3 + 0.07) + 0.07


def test_quantity_three_with_an_interval_that_is_no_multiple_of_dt():
    """Release times 1.0, 1.07, 1.14 (float64 +=) on the float32 clock 0, 0.05, ...: tick t's clock is t float32 additions of
    float32(0.05).  Written out: 1.0 <= clock(20) = 1.0000001 (clock(19) = 0.95000005 is short of it) -> tick 20; 1.07 <= clock(22) =
    1.1000001 (clock(21) = 1.0500001 is not) -> tick 22; 1.14 <= clock(23) = 1.1500001 -> tick 23."""
    traj, head, speeds = _lists(4, 2)
    sp = VehicleSpawner(traj, head, speeds, quantity=3, spawn_time=1.0, spawn_interval=0.07)
    assert release_times(sp).tolist() == [1.0, 1.0 + 0.07, (1.0 + 0.07) + 0.07]
    clock = [np.float32(0.0)]
    for _ in range(30):
        clock.append(np.float32(clock[-1] + np.float32(0.05)))
    assert clock[19] < 1.0 <= clock[20] and clock[21] < np.float32(1.07) <= clock[22] and clock[22] < np.float32(1.14) <= clock[23]
    tracks = tracks_from_spawners([sp], 0.05, 0.0)
    assert [t["first_tick"] for t in tracks] == [20, 22, 23]
    for t in tracks:                                   # every vehicle its own copy of all three lists (the quirk of :144 is not kept)
        assert np.array_equal(t["speed"], speeds[1:]) and np.array_equal(t["xy"], traj[1:]) and np.array_equal(t["yaw"], head[1:])
    assert len({id(t["speed"]) for t in tracks}) == 3


def test_one_release_per_spawner_per_tick():
    """An interval below the step length: VehicleSpawnManager.tick asks each spawner once per tick (vehicle_spawner.py:55-58), so
    the backlog leaves one per tick."""
    sp = VehicleSpawner(*_lists(3, 3), quantity=3, spawn_time=0.1, spawn_interval=0.01)
    assert [t["first_tick"] for t in tracks_from_spawners([sp], 0.05, 0.0)] == [2, 3, 4]


def test_a_spawn_time_behind_the_clock():
    """The reference's managers first run at the top of tick 0, on sim_time0: a spawner that is already due releases there
    (vehicle_spawner.py:183), one vehicle per tick.  A scenario that has already run 5 ticks when the tracks are set
    (elapsed_ticks) meets those vehicles under way: their first ticks are negative."""
    sp = VehicleSpawner(*_lists(40, 4), quantity=2, spawn_time=-1.0, spawn_interval=0.0)
    assert [t["first_tick"] for t in tracks_from_spawners([sp], 0.05, 2.0)] == [0, 1]
    tracks = tracks_from_spawners([sp], 0.05, 2.0, elapsed_ticks=5)
    assert [t["first_tick"] for t in tracks] == [-5, -4]
    # ... and tick 0 of the tracks sees keyframe 5 of the first vehicle: entry 6 of the spawner's lists
    sc = _scene(2)
    scenarios.place_tracked(sc, tracks, 0)
    assert np.array_equal(sc["dynamic_obstacles"][0][0], np.float32(tracks[0]["xy"][5]).astype(np.float64))


def test_a_spawn_time_exactly_on_a_clock_value():
    """<= (vehicle_spawner.py:183): a spawn time that IS the float32 clock of tick 7 releases in tick 7, the next float64 above it in
    tick 8 -- as long as it still rounds to another float32."""
    clock = np.float32(0.25)
    for _ in range(7):
        clock = np.float32(clock + np.float32(0.03))
    on = VehicleSpawner(*_lists(3, 5), quantity=1, spawn_time=float(clock), spawn_interval=1.0)
    above = VehicleSpawner(*_lists(3, 5), quantity=1, spawn_time=float(np.nextafter(clock, np.float32(np.inf))), spawn_interval=1.0)
    assert [t["first_tick"] for t in tracks_from_spawners([on, above], 0.03, 0.25)] == [7, 8]


def test_vehicles_and_pedestrians_of_one_spawn_time_enter_in_the_same_tick():
    for spawn_time, interval, dt, t0 in ((0.4, 0.07, 0.05, 0.0), (1.3, 0.01, 0.03, 0.25), (-2.0, 0.2, 0.05, 0.0)):
        ped = PedSpawner(np.zeros(3), np.array([[1.0, 0.0, 0.0]]), [False], 1.2, None, 3, spawn_time, interval, 1.5, 1.0)
        veh = VehicleSpawner(*_lists(5, 6), quantity=3, spawn_time=spawn_time, spawn_interval=interval)
        want, _ = birth_ticks(ped_release_times(ped).astype(np.float32), np.array([0, 1, 1]), t0, dt, 400)
        assert [t["first_tick"] for t in tracks_from_spawners([veh], dt, t0)] == want.tolist()
        assert first_ticks(release_times(veh), dt, t0) == want.tolist()


def test_keys_that_need_the_simulator_are_refused():
    traj, head, speeds = _lists(3, 7)
    with pytest.raises(ValueError, match="traffic manager or a BehaviorAgent"):
        VehicleSpawner(traj, head, speeds, auto_pilot=True)
    with pytest.raises(ValueError, match="recommended spawn points"):
        VehicleSpawner(traj, head, speeds, spawn_point=3)
    with pytest.raises(ValueError, match="recommended spawn points"):
        VehicleSpawner(traj, head, speeds, destination=1)
    with pytest.raises(ValueError, match="one entry per tick"):
        VehicleSpawner(traj, head[:2], speeds)
    with pytest.raises(ValueError, match="at least 2 entries"):
        VehicleSpawner(traj[:1], head[:1], speeds[:1])


# ---- place_tracked --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [(2.4, 1.0), (0.1, 0.1)])
def test_place_tracked_at_the_boundaries_of_a_track(ext):
    L, f = 4, 3
    sc = _scene(2, ext)
    free = (sc["dynamic_obstacles"][1][0].copy(), sc["dynamic_vel"][1].copy(), sc["dynamic_yaw"][1])
    tr = _track(L, f, 9)
    P = len(scenarios.ring_local_offsets(*ext))
    for d, present in ((-1, False), (0, True), (L - 1, True), (L, False)):
        s = dict(sc)
        scenarios.place_tracked(s, [tr, None], f + d)
        assert s["dynamic_present"].tolist() == [present, True]
        c, ring = s["dynamic_obstacles"][0]
        assert ring.shape == (P, 2)                                        # the point count of a ring never changes
        if present:
            assert np.array_equal(c, tr["xy"][d].astype(np.float32).astype(np.float64))
            assert np.array_equal(s["dynamic_vel"][0], np.float32(tr["speed"][d] * np.array([np.cos(tr["yaw"][d]), np.sin(tr["yaw"][d])])))
            assert s["dynamic_yaw"][0] == tr["yaw"][d]
            assert np.array_equal(ring, scenarios.place_ring_f32(c, tr["yaw"][d], scenarios.ring_local_offsets(*ext)))
            want = O.ellipse_ring(c, tr["yaw"][d], *ext)
            assert np.abs(ring - want).max() <= 4e-6 * max(1.0, np.abs(want).max())
        else:
            assert np.isposinf(c).all() and np.isposinf(ring).all() and not s["dynamic_vel"][0].any()
        # the untracked vehicle: where it was (no dt) ...
        assert np.array_equal(s["dynamic_obstacles"][1][0], free[0]) and np.array_equal(s["dynamic_vel"][1], free[1])
    # ... and one step of advance_dynamic's rule with dt
    s = dict(sc)
    scenarios.place_tracked(s, [tr, None], f, dt=0.04)
    assert np.array_equal(s["dynamic_obstacles"][1][0], scenarios.advance_center_f32(free[0], free[1], 0.04))
    assert np.array_equal(s["dynamic_obstacles"][1][1],
                          scenarios.place_ring_f32(s["dynamic_obstacles"][1][0], free[2], scenarios.ring_local_offsets(*ext)))


def test_an_absent_vehicle_fails_every_cull_and_never_refuses_a_gap():
    """The documented absent state in the arithmetic of the kernel's cull: d^2 = +inf is not < thr^2 for any threshold, an infinite
    one included; speed 0 is skipped by check_traffic (check_traffic.py:46)."""
    from carla_social_force_model_amd.check_traffic import check_traffic
    from carla_social_force_model_amd.host_state import PedMode, PedModeManager
    sc = _scene(1)
    scenarios.place_tracked(sc, [_track(2, 5)], 0)
    c = np.float32(sc["dynamic_obstacles"][0][0])
    with np.errstate(all="ignore"):
        for x in (np.float32(0.0), np.float32(3.0e15), np.float32(-3.0e38)):
            d2 = (x - c[0]) * (x - c[0]) + (x - c[1]) * (x - c[1])
            assert not d2 < np.float32(np.inf) and not d2 < np.float32(3.0e38)
        ped = {"loc": np.zeros(3), "next_waypoint": np.array([4.0, 0.0, 0.0]),
               "mode": PedModeManager("p", 1.2, PedMode.WALKING_SIDEWALK, 1.5, 1.0)}
        assert check_traffic(ped, sc["dynamic_obstacles"], sc["dynamic_vel"], sc["dynamic_extent"])


def test_place_tracked_takes_a_scenario_object_and_checks_counts():
    sc = scenarios.make_scenario(4, 5, n_dynamic=2)
    scenarios.place_tracked(sc, None, 3)
    assert sc.dynamic_present.all()
    with pytest.raises(ValueError, match="1 tracks for 2 vehicles"):
        scenarios.place_tracked(sc, [None], 0)


def test_make_track_plan_has_what_its_docstring_says():
    sc = _scene(4, n=64)
    ticks = 60
    tracks = scenarios.make_track_plan(sc, 3, ticks)
    pack_tracks([tracks], [sc])
    assert [t["first_tick"] for t in tracks] == [-2, 3, 6, 9]                                 # staggered entries
    ends = [t["first_tick"] + len(t["yaw"]) for t in tracks]
    assert min(ends) < ticks and max(ends) >= ticks                                          # an exit inside the run
    s0 = tracks[0]["speed"]
    stop = np.nonzero(s0 == 0.0)[0]
    assert len(stop) and s0[:stop[0]].max() > 0 and s0[stop[-1] + 1:].max() > 0              # brakes to 0 and pulls away
    assert all(t["speed"].max() <= 1.4 for t in tracks)
    for t in tracks:                                                                          # gentle arcs: the keyframes are a drive
        if len(t["yaw"]) > 1:
            assert np.abs(np.diff(t["yaw"])).max() < 0.05
            step = np.linalg.norm(np.diff(t["xy"], axis=0), axis=1)
            assert np.allclose(step, t["speed"][:-1] * 0.05, atol=1e-5)
    mid = sc["loc"][:, :2].mean(axis=0)
    assert all(np.linalg.norm(t["xy"] - mid, axis=1).min() < 2.0 for t in tracks)            # through the crowd


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi12_entry_points_are_declared():
    assert _lib.ABI_VERSION >= 12
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert int(re.search(r"#define SFM_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    assert int(re.search(r"#define SFM_BATCH_MAX_TRACK_KEYS \(1 << (\d+)\)", header).group(1)) == MAX_TRACK_KEYS.bit_length() - 1
    for name in ("sfm_batch_set_vehicle_tracks", "sfm_batch_download_vehicle_tracks"):
        assert name in _lib.SYMBOLS and _lib.SINCE[name] == 12
    assert len(_lib.SYMBOLS["sfm_batch_set_vehicle_tracks"][1]) == 9
    assert len(_lib.SYMBOLS["sfm_batch_download_vehicle_tracks"][1]) == 3
