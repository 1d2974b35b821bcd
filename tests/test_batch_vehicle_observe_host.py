"""CPU tests of the vehicle observations' host twin observe.observe_vehicles_scene: the record's rules at their edges -- exact
(d2, j) ties, fewer candidates than slots, the strict range test, the zero records, the three distances -- and frame 1 as a pure
function of the frame-0 record and the heading."""
import numpy as np
import pytest

import _driving_cases as D
from carla_social_force_model_amd import observe, scenarios
from carla_social_force_model_amd.scan import _fma32

H = observe.OBS_HEADER


def _scene(loc, vel=None, c=(0.0, 0.0), yaw=0.0, vvel=(0.5, 0.25), borders=(), statics=()):
    sc = D.one_vehicle_scene(c=c, yaw=yaw, vel=vvel)
    loc = np.asarray(loc, dtype=np.float64).reshape(-1, 2)
    sc["loc"] = np.column_stack((loc, np.zeros(len(loc))))
    sc["vel"] = np.zeros((len(loc), 3)) if vel is None else np.column_stack((np.asarray(vel, dtype=np.float64), np.zeros(len(loc))))
    sc["borders"], sc["static_obstacles"] = list(borders), list(statics)
    return sc


def test_exact_ties_go_to_the_lower_row():
    """Mirrored positions: d2 exactly equal in fp32; the slots hold ascending (d2, j)."""
    loc = [(3.0, 1.0), (1.0, 2.0), (-3.0, 1.0), (-1.0, -2.0), (3.0, -1.0), (2.0, 1.0), (0.5, 0.0)]
    vel = [(j + 1.0, -j) for j in range(len(loc))]
    rec = observe.observe_vehicles_scene(_scene(loc, vel), 6, 20.0)[0]
    order = [6, 1, 3, 5, 0, 2]                                         # d2: .25, 5, 5, 5, 10, 10 (row 4 ties too and comes last)
    assert rec[6] == 1.0 and rec[7] == 6
    for s, j in enumerate(order):
        want = np.float32([loc[j][0], loc[j][1], vel[j][0] - 0.5, vel[j][1] - 0.25])
        assert np.array_equal(rec[H + 4 * s:H + 4 * s + 4], want), (s, j)
    rec7 = observe.observe_vehicles_scene(_scene(loc, vel), 7, 20.0)[0]
    assert np.array_equal(rec7[H + 24:H + 26], np.float32(loc[4])) and np.array_equal(rec7[:H + 24], np.concatenate((rec[:7], [7], rec[8:])))


def test_fewer_candidates_than_slots_and_the_strict_range():
    loc = [(3.0, 4.0), (0.0, 1.0), (4.0, 3.0), (3.0e15, 0.0), (np.nan, 0.0), (0.0, 5.0)]     # d2 = 25 three times; a ghost; a NaN
    rec = observe.observe_vehicles_scene(_scene(loc), 4, 5.0)[0]                               # R2 = 25 exactly: 25 < 25 fails
    assert rec[7] == 1 and np.array_equal(rec[H:H + 2], np.float32([0.0, 1.0])) and not rec[H + 4:].any()
    rec = observe.observe_vehicles_scene(_scene(loc), 4, np.nextafter(np.float32(5.0), np.float32(6.0)))[0]
    assert rec[7] == 4 and np.array_equal(rec[H + 4:H + 16:4], np.float32([3.0, 4.0, 0.0]))   # rows 0, 2, 5 in index order
    assert observe.observe_vehicles_scene(_scene(np.zeros((0, 2))), 3, 5.0)[0, 7] == 0


def test_distances_flags_and_zero_records():
    line = np.float32([[x, 2.0] for x in np.arange(-3.0, 3.01, 0.5)])             # nearest to (0, 0): (0, 2), d2 = 4
    far = np.float32([[10.0, 10.0], [11.0, 10.0]])
    ring = scenarios.place_ring_f32((6.0, 0.0), 0.0, scenarios.ring_local_offsets(0.5, 0.5))
    sc = _scene([(0.0, 7.0), (3.0e15, 1.0)], borders=[far, line], statics=[(np.array([6.0, 0.0]), ring)], yaw=0.5)
    rec = observe.observe_vehicles_scene(sc, 2, 3.0, goals=[(5.0, -1.0)])[0]
    assert np.array_equal(rec[0:4], np.float32([5.0, -1.0, 0.5, 0.25]))
    assert np.array_equal(rec[4:6], scenarios.vehicle_headings(sc)[0]) and rec[6] == 1 and rec[7] == 0
    own = np.float32(sc["dynamic_obstacles"][0][1])
    d = own[:, None, :] - np.float32([[0.0, 7.0]])[None]
    assert rec[8] == observe._d2(-d[..., 0], -d[..., 1]).min() and 0 < rec[8] < 49       # the ring, not the centre; the ghost is out
    assert np.isposinf(rec[9])                                                           # no other vehicle
    assert np.array_equal(rec[10:12], np.float32([0.0, 2.0])) and not rec[12:14].any() and rec[14] == 1    # the ring is > 3 m away
    assert rec[15] == _fma32(np.float32(0.5), rec[4], np.float32(0.25) * rec[5])
    # two vehicles: other_d2; a mask; an absent vehicle
    sc["dynamic_obstacles"] = sc["dynamic_obstacles"] + [(np.array([3.0, 4.0]), ring), (np.array([np.inf, np.inf]), np.full_like(ring, np.inf))]
    sc["dynamic_vel"] = np.zeros((3, 2))
    sc["dynamic_yaw"], sc["dynamic_extent"] = np.zeros(3), np.ones((3, 2))
    rec = observe.observe_vehicles_scene(sc, 1, 3.0)
    assert rec[0, 9] == 25.0 and rec[1, 9] == 25.0 and not rec[2].any()
    rec = observe.observe_vehicles_scene(sc, 1, 3.0, mask=[0, 1, 1])
    assert not rec[0].any() and rec[1, 6] == 1.0 and not rec[2].any()
    sc["loc"], sc["vel"] = np.zeros((0, 3)), np.zeros((0, 3))
    assert np.isposinf(observe.observe_vehicles_scene(sc, 1, 3.0)[0, 8])                 # no live row


@pytest.mark.parametrize("yaw", [0.0, 0.9, -2.6])
def test_frame_1_is_a_pure_function_of_the_frame_0_record(yaw):
    rng = np.random.default_rng(3)
    made = vars(scenarios.make_scenario(40, 8, n_borders=2, n_static=2, n_dynamic=3))
    made["dynamic_yaw"] = made["dynamic_yaw"] + yaw
    goals = rng.uniform(0, 10, (3, 2))
    r0 = observe.observe_vehicles_scene(made, 5, 6.0, 0, goals=goals, mask=[1, 1, 0])
    r1 = observe.observe_vehicles_scene(made, 5, 6.0, 1, goals=goals, mask=[1, 1, 0])
    h = scenarios.vehicle_headings(made)
    assert np.array_equal(r1, observe.rotate_vehicle_record(r0, h), equal_nan=True) and r0[:2, 7].min() > 0
    keep = [4, 5, 6, 7, 8, 9, 14, 15]
    assert np.array_equal(r1[:, keep], r0[:, keep]) and not r1[2].any()
    for v in range(2):                                                     # the rule, spelled out on one 2-vector of each kind
        hx, hy = h[v]
        for c in (0, 2, 10, 12, H, H + 2, H + 18):
            p, q = r0[v, c], r0[v, c + 1]
            assert r1[v, c] == _fma32(hx, p, hy * q) and r1[v, c + 1] == _fma32(hx, q, -(hy * p))
        assert abs(np.hypot(*r1[v, 0:2].astype(np.float64)) - np.hypot(*r0[v, 0:2].astype(np.float64))) < 1e-5


def test_refused_settings():
    sc = _scene([(1.0, 1.0)])
    for kw in (dict(k=0), dict(k=17), dict(frame=2)):
        args = dict(k=2, sense_range=3.0, frame=0)
        args.update(kw)
        with pytest.raises(ValueError):
            observe.observe_vehicles_scene(sc, **args)
