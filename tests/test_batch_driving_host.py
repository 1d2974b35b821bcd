"""CPU tests of the driven vehicles' host side: the twin scenarios.drive_vehicles against the rule in include/sfm_hip.h (its edge
cases, and kinds that are not driven against today's twins bit for bit), what the bits mean over a long run (bounds derived in
_driving_cases.py), and the packers and refusals that need no GPU."""
import copy
import os
from types import SimpleNamespace

import numpy as np
import pytest

import _driving_cases as D
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd import batch as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _h(sc):
    return sc["dynamic_heading"][0].copy()


def test_a_zero_velocity_command_keeps_the_heading():
    sc = D.one_vehicle_scene(yaw=0.7, vel=(1.0, 2.0))
    h0 = scenarios.vehicle_headings(sc)[0]
    c0 = sc["dynamic_obstacles"][0][0].copy()
    scenarios.drive_vehicles(sc, 1, np.zeros(3, np.float32), 0.05)
    assert np.array_equal(_h(sc), h0) and not sc["dynamic_vel"].any()
    assert np.array_equal(sc["dynamic_obstacles"][0][0], c0)                   # v' = 0: the centre stays, the old velocity is gone
    scenarios.drive_vehicles(sc, 1, np.float32([0.0, -3.0, 9.0]), 0.05)      # c is ignored; the heading turns to v' / |v'|
    assert np.array_equal(_h(sc), np.float32([0.0, -1.0])) and np.array_equal(sc["dynamic_vel"][0], [0.0, -3.0])


def test_a_degenerate_turn_keeps_the_heading():
    sc = D.one_vehicle_scene(yaw=-2.1)
    h0 = scenarios.vehicle_headings(sc)[0]
    scenarios.drive_vehicles(sc, 2, np.float32([2.0, 0.0, 0.0]), 0.05)       # (b, c) = 0: g = 0, n2 == 0
    assert np.array_equal(_h(sc), h0)
    assert np.array_equal(sc["dynamic_vel"][0], (np.float32(2.0) * h0).astype(np.float64))


def test_a_negative_speed_reverses():
    sc = D.one_vehicle_scene(yaw=0.0)
    c0 = sc["dynamic_obstacles"][0][0].copy()
    scenarios.drive_vehicles(sc, 2, np.float32([-4.0, 1.0, 0.0]), 0.05)
    assert np.array_equal(_h(sc), np.float32([1.0, 0.0]))                      # the heading stays forward
    assert np.array_equal(sc["dynamic_vel"][0], [-4.0, 0.0])
    assert sc["dynamic_obstacles"][0][0][0] < c0[0] and sc["dynamic_obstacles"][0][0][1] == c0[1]


@pytest.mark.parametrize("kind", [1, 2])
def test_a_centre_that_is_not_finite_stays_absent(kind):
    for bad in (np.inf, np.nan):
        sc = D.one_vehicle_scene(yaw=0.4)
        h0 = scenarios.vehicle_headings(sc)[0]
        sc["dynamic_obstacles"] = [(np.array([bad, 1.0]), sc["dynamic_obstacles"][0][1])]
        scenarios.drive_vehicles(sc, kind, np.float32([1.0, 0.6, 0.8]), 0.05)
        c, ring = sc["dynamic_obstacles"][0]
        assert np.isposinf(c).all() and np.isposinf(ring).all() and ring.shape == (68, 2)
        assert not sc["dynamic_vel"].any() and np.array_equal(_h(sc), h0) and not sc["dynamic_present"][0]


@pytest.mark.parametrize("kind", [0, 3])
def test_kinds_that_are_not_driven_equal_todays_twins(kind):
    """Free running against advance_dynamic, tracked against place_tracked, bit for bit over 6 ticks."""
    made = scenarios.make_scenario(0, 41, n_dynamic=5)
    sc = {k: copy.deepcopy(v) for k, v in vars(made).items()}
    ref = SimpleNamespace(**copy.deepcopy(sc))
    for _ in range(6):
        scenarios.drive_vehicles(sc, kind, np.float32([1.0, 1.0, 0.0]), 0.04)
        scenarios.advance_dynamic(ref, 0.04)
        for (c, r), (c2, r2) in zip(sc["dynamic_obstacles"], ref.dynamic_obstacles):
            assert np.array_equal(c, c2) and np.array_equal(r, r2)
    rng = np.random.default_rng(5)
    L = 4
    yaw = rng.uniform(-3, 3, L)
    track = {"xy": rng.uniform(0, 9, (L, 2)), "yaw": yaw, "speed": rng.uniform(0.2, 1.4, L), "first_tick": 1}
    tracks = [track, None, None, None, None]
    a = {k: copy.deepcopy(v) for k, v in vars(made).items()}
    b = copy.deepcopy(a)
    D.start_twin([a], [tracks])
    scenarios.place_tracked(b, tracks, 0, None)
    h0 = a["dynamic_heading"].copy()
    for tau in range(1, 7):                                                    # absent, four keyframes, absent again
        scenarios.drive_vehicles(a, kind, np.zeros(3, np.float32), 0.04, tracks, tau)
        scenarios.place_tracked(b, tracks, tau, 0.04)
        for (c, r), (c2, r2) in zip(a["dynamic_obstacles"], b["dynamic_obstacles"]):
            assert np.array_equal(c, c2) and np.array_equal(r, r2), tau
        assert np.array_equal(a["dynamic_vel"], b["dynamic_vel"]) and np.array_equal(a["dynamic_present"], b["dynamic_present"])
    assert np.array_equal(a["dynamic_heading"], h0)                            # nothing that is not driven turns a heading


def test_what_the_bits_mean_over_2000_ticks():
    """A kind 2 vehicle for 2 000 ticks, turns and speeds of both signs: |h|^2 - 1 inside the bound of one normalisation at every
    tick, the centre inside the derived bound of the same scheme in float64 at every tick."""
    T, dt = 2000, 0.05
    cmds = D.turn_commands(T, 11)
    assert (cmds[:, 0] < 0).any() and (cmds[:, 0] > 0).any() and (cmds[:, 2] < 0).any() and (cmds[:, 2] > 0).any()
    sc = D.one_vehicle_scene(c=(12.5, -40.25), yaw=1.1)
    h0 = scenarios.vehicle_headings(sc)[0]
    c64, h64 = D.unicycle64(sc["dynamic_obstacles"][0][0], h0, cmds, dt)
    cmax = np.abs(c64).max() + 1.0
    worst_h = worst_c = 0.0
    for t in range(T):
        scenarios.drive_vehicles(sc, 2, cmds[t], dt)
        h = _h(sc).astype(np.float64)
        worst_h = max(worst_h, abs(h[0] * h[0] + h[1] * h[1] - 1.0))
        err = np.abs(sc["dynamic_obstacles"][0][0] - c64[t + 1]).max()
        bound = D.centre_bound(dt, cmds[:t + 1, 0], cmax)
        worst_c = max(worst_c, err / bound)
        assert err <= bound, (t, err, bound)
    print(f"worst | |h|^2 - 1 | = {worst_h:.3e} (bound {D.H2_BOUND:.3e}); worst centre error / bound = {worst_c:.3f}; "
          f"final bound {D.centre_bound(dt, cmds[:, 0], cmax):.3e} m")
    assert worst_h <= D.H2_BOUND
    assert np.abs(c64).max() < cmax


def test_packers():
    io = np.array([0, 2, 2, 5], np.int32)
    kd, a, b, c = B.pack_vehicle_driving([[1, 2], None, 0], [np.float32([[1, 2, 3], [4, 5, 6]]), None, np.float32([7, 8, 9])], io)
    assert kd.dtype == np.uint8 and kd.tolist() == [1, 2, 0, 0, 0]
    assert a.tolist() == [1, 4, 7, 7, 7] and b.tolist() == [2, 5, 8, 8, 8] and c.tolist() == [3, 6, 9, 9, 9]
    kd, a, b, c = B.pack_vehicle_driving(None, np.zeros((5, 3)), io)
    assert kd is None and a.shape == (5,)
    kd, a, _, _ = B.pack_vehicle_driving(2, None, io)
    assert kd.tolist() == [2] * 5 and not a.any()
    k, r, frame, gx, gy, mk = B.vehicle_observation_arrays(io, 4, 5.0, 1, goals=[None, None, np.float32([1, 2])], mask=[1, 0, 1])
    assert (k, frame) == (4, 1) and r.tolist() == [5.0] * 3 and gx.tolist() == [0, 0, 1, 1, 1] and gy.tolist() == [0, 0, 2, 2, 2]
    assert mk.dtype == np.uint8 and mk.tolist() == [1, 1, 1, 1, 1]
    assert B.vehicle_observation_arrays(io, 1, [1, 2, 3], 0)[3:] == (None, None, None)


def test_refusals_without_a_gpu():
    io = np.array([0, 2, 3], np.int32)
    for bad in ([[1, 3], 0], np.array([1, 2]), [[1, 2]]):
        with pytest.raises(ValueError):
            B.pack_vehicle_driving(bad, None, io)
    with pytest.raises(ValueError):
        B.pack_vehicle_driving(1, np.zeros((3, 2)), io)
    with pytest.raises(ValueError, match="finite"):
        B.pack_vehicle_driving([[1, 0], 0], np.float32([[np.inf, 0, 0], [0, 0, 0], [0, 0, 0]]), io)
    B.pack_vehicle_driving([[0, 1], 0], np.float32([[np.inf, 0, 0], [0, 0, 0], [np.nan, 0, 0]]), io)   # not driven: anything goes
    with pytest.raises(ValueError, match="finite"):
        B.pack_vehicle_driving(None, np.float32([[np.nan, 0, 0], [0, 0, 0], [0, 0, 0]]), io)
    for kw in (dict(k=0), dict(k=17), dict(frame=2), dict(sense_range=0.0), dict(sense_range=np.inf), dict(sense_range=2e6),
               dict(goals=np.float32([np.nan, 0])), dict(goals=np.zeros((2, 2))), dict(mask=[1, 1, 1])):
        args = dict(k=4, sense_range=5.0, frame=0, goals=None, mask=None)
        args.update(kw)
        with pytest.raises(ValueError):
            B.vehicle_observation_arrays(io, **args)


def test_the_binding_and_the_header_agree():
    names = {"sfm_batch_set_vehicle_driving": 5, "sfm_batch_set_vehicle_commands": 4, "sfm_batch_download_vehicle_driving": 9,
             "sfm_batch_set_vehicle_observation": 7, "sfm_batch_observe_vehicles": 1, "sfm_batch_download_vehicle_observations": 2}
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    for name, nargs in names.items():
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs and _lib.SINCE[name] == 17
        assert name in _lib.UNBUMPED                                     # an older build of the same ABI number still loads
        assert f"int {name}(SfmBatch* b" in header
    assert "#define SFM_BATCH_PTR_VEHICLE_COMMANDS 10" in header and "#define SFM_BATCH_PTR_VEHICLE_OBS 11" in header
    assert (B.PTR_VEHICLE_COMMANDS, B.PTR_VEHICLE_OBS) == (10, 11) and _lib.ABI_VERSION == 17
    assert (B.DRIVE_OFF, B.DRIVE_VELOCITY, B.DRIVE_UNICYCLE) == (0, 1, 2)
