"""CPU tests of the vehicle episodes' host side: the NumPy twins ``episode.box_gap2`` / ``episode.vehicle_episode_scene`` and
``scenarios.respawn_vehicles_scene``, the float64 statement they are held against, and the bound between the two
(tests/_vehicle_episode_cases.py derives it).  The GPU tests hold the device against the twins bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

import _driving_cases as DC
import _vehicle_episode_cases as VC
from carla_social_force_model_amd import episode, observe, scenarios
from carla_social_force_model_amd.batch import vehicle_episode_arrays

INF = np.float32(np.inf)
F = np.float32


# ---- H1: hand values ----------------------------------------------------------------------------------------------------------------

def test_box_gap2_equals_hand_values_on_a_dyadic_axis_aligned_box():
    pts = np.array([[4.0, 2.0], [4.0, 4.5], [1.5, 2.25], [3.0, 2.0], [3.0, 3.0], [-2.5, 0.0], [1.0, -0.5], [1.0e13, 0.0], [np.nan, 0.0]])
    got = episode.box_gap2((1.0, 2.0), (1.0, 0.0), (2.0, 1.0), pts)
    want = np.array([1.0, 1.0 + 2.25, 0.0, 0.0, 0.0, 2.25 + 1.0, 2.25, np.inf, np.inf], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # the same box turned a quarter: (0, 1) swaps the roles of the axes, exactly
    got = episode.box_gap2((1.0, 2.0), (0.0, 1.0), (2.0, 1.0), np.array([[1.0, 6.0], [3.5, 2.0], [1.5, 3.75]]))
    assert np.array_equal(got, np.array([4.0, 2.25, 0.0], np.float32))


def _one(ped_x, ped_radius, ped_y=2.0):
    """One vehicle at (1, 2), heading (1, 0), half-extents (2, 1), and one pedestrian."""
    sc = {"loc": np.array([[ped_x, ped_y, 0.0]]), "vel": np.zeros((1, 3)),
          "dynamic_obstacles": [(np.array([1.0, 2.0]), np.zeros((0, 2)))], "dynamic_heading": np.array([[1.0, 0.0]], np.float32)}
    return episode.vehicle_episode_scene(sc, True, [[50.0, 2.0]], [[2.0, 1.0]], (0.0, ped_radius, 0.0, 0.0), 0)


def test_every_decision_is_a_strict_less_than():
    rec, done, scene_done, _, _ = _one(3.0, 0.5)                        # exactly on the box edge: gap 0
    assert rec[0, episode.EP_PED_GAP2] == 0.0 and rec[0, episode.EP_REASON] == episode.REASON_PED_HIT and done[0] and scene_done
    rec, done, scene_done, _, _ = _one(3.5, 0.5)                        # exactly at the radius: 0.25 < 0.25 is false
    assert rec[0, episode.EP_PED_GAP2] == 0.25 and rec[0, episode.EP_REASON] == 0 and not done[0] and not scene_done
    inside = np.nextafter(F(3.5), F(0.0))                               # one ulp inside: every operation on the way is exact
    rec, done, _, _, _ = _one(float(inside), 0.5)
    assert rec[0, episode.EP_PED_GAP2] < 0.25 and rec[0, episode.EP_REASON] == episode.REASON_PED_HIT and done[0]
    for x in (3.0, 1.0):                                                # a radius of 0 never fires: on the edge, inside the box
        rec, done, _, _, _ = _one(x, 0.0)
        assert rec[0, episode.EP_PED_GAP2] == 0.0 and rec[0, episode.EP_REASON] == 0 and not done[0]


# ---- H2: why the box test exists ----------------------------------------------------------------------------------------------------

def _ring_and_box(ped, radius=0.3):
    """(clear_d2 of the vehicle observation, ped_gap2 of the vehicle record, r2) for one vehicle at the origin, heading (1, 0)."""
    c, h = np.zeros(2), np.array([1.0, 0.0], np.float32)
    ring = scenarios.place_ring_heading_f32(c, h, scenarios.ring_local_offsets(*VC.EXTENT))
    sc = {"loc": np.array([[ped[0], ped[1], 0.0]]), "vel": np.zeros((1, 3)), "waypoint": np.zeros((1, 3)), "dynamic_obstacles": [(c, ring)],
          "dynamic_heading": h.reshape(1, 2), "dynamic_vel": np.zeros((1, 2))}
    clear = observe.observe_vehicles_scene(sc, 1, 50.0)[0, 8]
    rec = episode.vehicle_episode_scene(sc, True, [[50.0, 0.0]], [VC.EXTENT], (0.0, radius, 0.0, 0.0), 0)[0]
    return clear, rec[0, episode.EP_PED_GAP2], episode.radius2(radius)


def test_ring_points_and_box_disagree_on_a_flank_between_ring_samples():
    clear, gap2, r2 = _ring_and_box((0.155, 1.05))                      # 5 cm off the flank, between the two samples beside th = 90 degrees
    assert gap2 < r2 <= clear, (clear, gap2)                            # the box: a contact; the ring points: clear


def test_ring_points_and_box_disagree_near_a_corner():
    clear, gap2, r2 = _ring_and_box((2.8, 0.8))                         # on the ellipse, 40 cm in front of the body
    assert clear < r2 <= gap2, (clear, gap2)                            # the ring points: a hit; the box: clear
    assert abs(float(gap2) - 0.16) < 1e-6


# ---- H3: the twin against the float64 statement -------------------------------------------------------------------------------------

def test_the_bound_is_the_one_derived():
    u = 2.0 ** -24
    assert VC.H2 == DC.H2_BOUND                                         # the drift of a driven heading
    e3 = (1 + u) ** 3 - 1
    dh = VC.H2 / 2 + VC.H2 ** 2 / 8
    eu = e3 * (1 + dh) + dh
    ea = eu + u * (1 + eu)
    es = ea * (2 * np.sqrt(2.0) + 2 * ea)
    assert VC.GAP2_REL == es + (2 * u + u * u) * (1 + es)
    assert 21.0 * u < VC.GAP2_REL < 23.0 * u
    for sc in VC.scenes():                                              # the headings of the cases are inside the drift the bound assumes
        h = np.asarray(sc["dynamic_heading"], dtype=np.float64).reshape(-1, 2)
        assert (np.abs((h * h).sum(axis=1) - 1.0) <= VC.H2).all()
    assert tuple(VC.scenes()[VC.UP_SCENE]["dynamic_heading"][VC.UP_VEHICLE]) == (0.0, 1.0)


def _candidates(sc, v):
    rows = np.asarray(sc["loc"], dtype=np.float64).reshape(-1, 3)[:, :2]
    rings = [r for q, (_, r) in enumerate(sc["dynamic_obstacles"]) if q != v]
    other = np.concatenate(rings) if rings else np.zeros((0, 2))
    wall = [np.asarray(p) for p in sc["borders"]] + [np.asarray(r) for _, r in sc["static_obstacles"]]
    return rows, other, (np.concatenate(wall) if wall else np.zeros((0, 2)))


@pytest.mark.parametrize("k", range(VC.B))
def test_the_three_gaps_against_a_float64_point_to_rectangle_distance(k):
    sc = VC.absent_scene(k)
    rec = VC.twin(k)[0]
    checked = 0
    for v in np.flatnonzero(VC.agents()[k]):
        c, h, e = sc["dynamic_obstacles"][v][0], sc["dynamic_heading"][v], VC.EXTENT
        if not np.isfinite(c).all():
            continue
        for slot, pts in zip((episode.EP_PED_GAP2, episode.EP_VEH_GAP2, episode.EP_WALL_GAP2), _candidates(sc, v)):
            f = episode.box_gap2(c, h, e, pts)
            got = np.float32(f.min()) if f.size else INF
            assert got == rec[v, slot] or (np.isinf(got) and np.isinf(rec[v, slot]))       # the record's slot is this minimum
            g64, r2 = VC.rect_gap2_64(c, h, e, pts)
            if not np.isfinite(g64).any():
                assert np.isinf(got), (k, v, slot)                        # no live candidate: +inf on both sides
                checked += 1
                continue
            i, j = int(np.argmin(g64)), int(np.argmin(f))
            bound = VC.GAP2_REL * max(r2[i], r2[j])
            print(f"scene {k} vehicle {v} slot {slot}: |{float(got):.9g} - {g64[i]:.9g}| = {abs(float(got) - g64[i]):.3g} <= {bound:.3g}")
            assert abs(float(got) - g64[i]) <= bound, (k, v, slot)
            checked += 1
    assert checked == 3 * sum(bool(np.isfinite(sc["dynamic_obstacles"][v][0]).all()) for v in np.flatnonzero(VC.agents()[k]))


def test_an_absent_ring_beside_a_heading_with_a_zero_component_is_no_contact():
    k, v = VC.UP_SCENE, VC.UP_VEHICLE
    sc = VC.absent_scene(k)
    ring = sc["dynamic_obstacles"][VC.ABSENT[k]][1]
    assert np.isinf(ring).all()
    with np.errstate(invalid="ignore"):                                 # what the rule keeps out: inf * 0 is NaN, fmax(NaN - e, 0) is 0
        assert np.isnan(np.float32(0.0) * np.float32(np.inf)) and np.fmax(np.float32(np.nan) - np.float32(1.0), np.float32(0.0)) == 0.0
    rec = VC.twin(k)[0]
    assert np.isinf(rec[v, episode.EP_VEH_GAP2]) and not int(rec[v, episode.EP_REASON]) & episode.REASON_VEH_HIT


# ---- H4: the state machine ----------------------------------------------------------------------------------------------------------

def test_an_agent_that_is_not_live_gets_reason_16_and_the_prev_it_holds_stays():
    k, v = 8, VC.ABSENT[8]
    prevs = np.full(VC.VEHICLES[k], 7.5, np.float32)
    rec, done, scene_done, ages, prevs2 = VC.twin(k, ages=np.array([4, 9]), prevs=prevs)
    assert rec[v, episode.EP_REASON] == episode.REASON_NOT_LIVE and rec[v, episode.EP_DONE] == 1.0 and done[v] and scene_done
    assert rec[v, episode.EP_AGE] == 5.0 and np.isinf(rec[v, 3:]).all() and (rec[v, 3:] > 0).all()
    assert prevs2[v] == F(7.5) and ages[v] == 5
    other = 1 - v                                                       # not an agent: zeros, state as given
    assert not rec[other].any() and not done[other] and ages[other] == 9 and prevs2[other] == F(7.5)


def test_time_limit_and_prev_goal_d2():
    k = 1                                                               # max_steps 2, goal radius 0
    assert VC.MAX_STEPS[k] == 2
    r1, _, _, ages, prevs = VC.twin(k)
    assert r1[0, episode.EP_AGE] == 1.0 and not int(r1[0, episode.EP_REASON]) & episode.REASON_TIME_LIMIT
    assert r1[0, episode.EP_PREV_GOAL_D2] == r1[0, episode.EP_GOAL_D2] and prevs[0] == r1[0, episode.EP_GOAL_D2]    # the first evaluation
    moved = [(np.array([0.5, 0.25]) + VC.scenes()[k]["dynamic_obstacles"][0][0], VC.scenes()[k]["dynamic_obstacles"][0][1])]
    r2, done, _, ages, prevs = VC.twin(k, vehicles=moved, ages=ages, prevs=prevs)
    assert r2[0, episode.EP_AGE] == 2.0 and int(r2[0, episode.EP_REASON]) & episode.REASON_TIME_LIMIT and done[0]
    assert r2[0, episode.EP_PREV_GOAL_D2] == r1[0, episode.EP_GOAL_D2] and r2[0, episode.EP_GOAL_D2] != r1[0, episode.EP_GOAL_D2]
    assert prevs[0] == r2[0, episode.EP_GOAL_D2] and ages[0] == 2


def test_every_reason_fires_somewhere_in_the_cases():
    reasons = 0
    for k in range(VC.B):
        ages = prevs = None
        for _ in range(3):
            rec, _, _, ages, prevs = VC.twin(k, ages=ages, prevs=prevs)
            for r in rec[VC.agents()[k], episode.EP_REASON]:
                reasons |= int(r)
    assert reasons == 1 | 2 | 4 | 8 | 16 | 32, reasons


def test_settings_are_validated_on_the_host():
    io = np.array([0, 2, 3], np.int32)
    ag, gx, gy, ex, rg, rp, rv, rw, ms = vehicle_episode_arrays(io, [[1, 0], [1]], np.zeros((3, 2)), np.array([2.4, 1.0]), 1.0, 0.5, 0.0, [0.2, 0.3], 7)
    assert ag.tolist() == [1, 0, 1] and ex.shape == (3, 2) and ex.dtype == np.float32 and rw.tolist() == [F(0.2), F(0.3)] and ms.tolist() == [7, 7]
    with pytest.raises(ValueError):
        vehicle_episode_arrays(io, True, np.zeros((3, 2)), np.array([2.4, 0.0]))                  # an agent's extent must be > 0
    vehicle_episode_arrays(io, [[0, 1], [1]], np.zeros((3, 2)), np.array([[0.0, 0.0], [1.0, 1.0], [1.0, 1.0]]))     # ... not the others'
    with pytest.raises(ValueError):
        vehicle_episode_arrays(io, True, np.full((3, 2), np.inf), np.array([2.4, 1.0]))
    with pytest.raises(ValueError):
        vehicle_episode_arrays(io, True, np.zeros((3, 2)), np.array([2.4, 1.0]), wall_radius=-1.0)


# ---- H5: the respawn twin -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("choice", ["none", "one", "all", "third"])
def test_the_respawn_twin_leaves_everything_but_the_chosen_vehicles_alone(choice):
    rng = np.random.default_rng(77)
    M = 7
    mk = lambda: {"centers": rng.normal(size=(M, 2)), "vel": rng.normal(size=(M, 2)), "headings": rng.normal(size=(M, 2)),
                  "rings": [rng.normal(size=(3 + q, 2)) for q in range(M)], "cursor": rng.integers(0, 9, M)}
    snap, now = mk(), mk()
    now["age"], now["prev"], now["clock"] = np.arange(M) + 3, rng.uniform(1, 2, M).astype(np.float32), 12.5
    ch = {"none": np.zeros(M, bool), "one": np.arange(M) == 4, "all": np.ones(M, bool), "third": np.arange(M) % 3 == 0}[choice]
    out = scenarios.respawn_vehicles_scene(ch, snap, now)
    for key in ("centers", "vel", "headings", "cursor"):
        assert np.array_equal(out[key][ch], snap[key][ch]) and np.array_equal(out[key][~ch], now[key][~ch])
    for q in range(M):
        assert np.array_equal(out["rings"][q], (snap if ch[q] else now)["rings"][q])
    assert (out["age"][ch] == 0).all() and np.isnan(out["prev"][ch]).all()
    assert np.array_equal(out["age"][~ch], now["age"][~ch]) and np.array_equal(out["prev"][~ch], now["prev"][~ch])
    assert out["clock"] == 12.5 and np.array_equal(now["age"], np.arange(M) + 3)        # the input is not changed


def test_the_example_imports_without_a_gpu():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "batch_av_episode_loop.py")
    spec = importlib.util.spec_from_file_location("batch_av_episode_loop", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main)
