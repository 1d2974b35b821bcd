"""Host tests of the batch's vehicle autopilot: the NumPy twin (autopilot.autopilot_vehicle / autopilot_scene) against the float64
restatement of its speed rule inside bounds derived in _autopilot_cases.py, the leader's choice at exact ties and strict edges, the
cursor, the turn, what the rule means over a few hundred ticks (the twin plus scenarios.drive_vehicles), the packing, and the ABI.
No GPU."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import _autopilot_cases as AC
import _driving_cases as D
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd import autopilot as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "carla-social-force-model_amd", "csrc")
IO1 = np.array([0, 1])
F = np.float32


def _st(**kw):
    loop, ign = kw.pop("loop", False), kw.pop("ignore_walkers", False)
    st, fl = A.pack_settings(IO1, loop=loop, ignore_walkers=ign, **kw)
    return st[0], int(fl[0])


# exactly representable geometry: a vehicle at the origin heading +x, so al = x and ac = -y exactly
EDGE = dict(v0=8.0, T=1.0, s0=2.0, acc=1.5, dec=2.0, brake=6.0, half_width=1.0, front=2.0, look=16.0, reach=1.0, ped_margin=0.5, max_turn=0.05)


def _one(peds, path=((100.0, 0.0),), others=(), vel=(1.0, 0.0), cursor=0, **kw):
    st, fl = _st(**dict(EDGE, **kw))
    sc = AC.street([((0.0, 0.0), 0.0, vel)] + list(others))
    ctr, v, h, rings = A.scene_vehicles(sc)
    pk = np.zeros((len(peds), 4), F)
    pk[:, :np.shape(peds)[1] if len(peds) else 0] = peds
    return A.autopilot_vehicle(0, ctr, v, h, rings, pk, np.array(path), st, fl, cursor, 0.05)


def test_the_twin_stays_within_the_derived_bound_of_the_float64_rule():
    """4000 draws of (s, u, gap, settings): |s'_twin - s'_f64| inside the bound derived from the roundings of step 5; the draws within
    that bound of a max / clamp switch are left out, and they are at most 1 % -- counted on the float64 restatement alone."""
    draws = AC.draws(4000, 11)
    out = sum(AC.near_a_switch(*d) for d in draws)
    assert out <= 0.01 * len(draws), out
    worst = 0.0
    for s, u, gap, led, st, dt in draws:
        if AC.near_a_switch(s, u, gap, led, st, dt):
            continue
        a32, s32 = A.idm_speed(s, u, gap, led, st, dt)
        a64, s64 = A.idm_f64(s, u, gap, led, st, dt)
        bound = AC.speed_terms(s, u, gap, led, st, dt)[3]
        assert abs(float(s32) - s64) <= bound, (s, u, gap, led, st, dt, s32, s64, bound)
        worst = max(worst, abs(float(s32) - s64) / bound)
    assert worst > 0.01                                                  # (the bound is not vacuous: some draw uses a part of it)


def test_the_leader_is_the_minimum_of_gap_kind_index():
    # two pedestrians at the same gap: the lower row
    cmd, cur, rec = _one([(10.0, 0.5), (10.0, -0.5)])
    assert (rec[1], rec[2], rec[3]) == (1, 0, 7.5)
    cmd, cur, rec = _one([(12.0, 0.0), (10.0, 0.5), (10.0, -0.5)])
    assert (rec[1], rec[2]) == (1, 1)
    # a pedestrian and the end of the path at the same gap: the lower kind; the end nearer: kind 3
    cmd, cur, rec = _one([(10.0, 0.0)], path=((7.5, 0.0),))
    assert (rec[1], rec[3]) == (1, 7.5)
    cmd, cur, rec = _one([(10.0, 0.0)], path=((7.0, 0.0),))
    assert (rec[1], rec[2], rec[3], rec[4]) == (3, 0, 7.0, 0.0)
    # a pedestrian and a ring point of another vehicle at exactly the same gap: the lower kind; the ring nearer by one ulp: kind 2
    ahead = ((20.0, 0.0), 0.0, (2.0, 0.0))
    gv = _one([], others=[ahead])[2][3]
    x = F(F(gv + F(0.5)) + F(2.0))
    assert F(F(x - F(2.0)) - F(0.5)) == gv                               # (the pedestrian's gap is the ring's, exactly)
    cmd, cur, rec = _one([(x, 0.0)], others=[ahead])
    assert (rec[1], rec[2], rec[3], rec[4]) == (1, 0, gv, 0.0)
    cmd, cur, rec = _one([(np.nextafter(x, F(100)), 0.0)], others=[ahead])
    assert (rec[1], rec[2], rec[3], rec[4]) == (2, 1, gv, 2.0)
    # two vehicles at exactly the same gap (the same place): the lower index, and its speed
    for others, u in (([ahead, ((20.0, 0.0), 0.0, (1.0, 0.0))], 2.0), ([((20.0, 0.0), 0.0, (1.0, 0.0)), ahead], 1.0)):
        cmd, cur, rec = _one([], others=others)
        assert (rec[1], rec[2], rec[3], rec[4]) == (2, 1, gv, u)
    # dead rows are never leaders: parked where the library parks them (despawned, unborn), or not a number
    cmd, cur, rec = _one([(1.0e30, 0.0), (np.nan, 0.0), (3.0e12, 0.1), (12.0, 0.0)])
    assert (rec[1], rec[2]) == (1, 3)
    cmd, cur, rec = _one([(1.0e30, 1.0e30), (np.inf, 0.0)], loop=True)
    assert rec[1] == 0 and not rec[2:5].any()


def test_the_corridor_edges_are_strict():
    half, fl_ = 1.5, 18.0                                                # half_width + ped_margin, front + look: exact
    for ped, kind in (((0.0, 0.0), 0), ((2.0 ** -20, 0.0), 1), ((5.0, half), 0), ((5.0, -half), 0), ((5.0, float(np.nextafter(F(half), F(0)))), 1),
                      ((fl_, 0.0), 0), ((float(np.nextafter(F(fl_), F(0))), 0.0), 1), ((-3.0, 0.0), 0)):
        assert _one([ped], loop=True)[2][1] == kind, ped
    assert _one([(5.0, 0.2)], ignore_walkers=True, loop=True)[2][1] == 0
    # a negative gap (inside front + margin) is floored, not dropped
    cmd, cur, rec = _one([(1.0, 0.0)])
    assert rec[1] == 1 and rec[3] == -1.5 and rec[5] == -EDGE["brake"]


def test_rings_of_the_other_vehicles():
    ahead = ((20.0, 0.0), 0.0, (2.0, 0.5))
    cmd, cur, rec = _one([], others=[ahead])
    ring = scenarios.place_ring_f32(np.array([20.0, 0.0]), 0.0, scenarios.ring_local_offsets(2.4, 1.0))
    inside = ring[np.abs(ring[:, 1]) < 1.0]
    assert rec[1] == 2 and rec[2] == 1 and rec[3] == F(F(inside[:, 0].min()) - F(2.0)) and rec[4] == 2.0
    # the vehicle's own ring is never a candidate: alone, its ring points ahead of the bumper lead nowhere
    own = scenarios.ring_local_offsets(2.4, 1.0)
    assert (own[:, 0] > 2.0).any() and _one([], loop=True)[2][1] == 0
    # an absent other vehicle (centre and ring at +inf) is no candidate; a nearer one behind it is
    sc = AC.street([((0.0, 0.0), 0.0, (1.0, 0.0)), ahead, ((15.0, 0.0), 0.0, (0.0, 0.0))])
    sc["dynamic_obstacles"][1] = (np.full(2, np.inf), np.full_like(sc["dynamic_obstacles"][1][1], np.inf))
    st, fl = A.pack_settings(np.array([0, 3]), **EDGE)
    cmds, cur, rec = A.autopilot_scene(sc, None, [np.array([[100.0, 0.0]]), None, None], st, fl, np.zeros(3, int), 0.05)
    assert rec[0, 1] == 2 and rec[0, 2] == 2
    assert not cmds[1:].any() and not rec[1:].any()                      # P_k = 0: the caller's commands are left alone
    keep = np.float32([[9, 9, 9, 9], [1, 2, 3, 1], [4, 5, 6, 2]])
    cmds, _, _ = A.autopilot_scene(sc, None, [np.array([[100.0, 0.0]]), None, None], st, fl, np.zeros(3, int), 0.05, keep)
    assert np.array_equal(cmds[1:], keep[1:]) and cmds[0, 3] == 2


def test_the_cursor():
    r = 1.0                                                              # reach2 = 1
    # strict <: a waypoint at exactly reach is kept, one just inside is passed
    assert _one([], path=((1.0, 0.0), (5.0, 0.0)))[1] == 0
    assert _one([], path=((float(np.nextafter(F(r), F(0))), 0.0), (5.0, 0.0)))[1] == 1
    # several points inside reach in one launch
    assert _one([], path=((0.1, 0.0), (0.2, 0.1), (-0.3, 0.2), (9.0, 0.0), (0.0, 0.0)))[1] == 3
    # a loop wraps, and steps at most P times when every point is inside reach
    assert _one([], path=((9.0, 0.0), (0.1, 0.0), (0.2, 0.0)), cursor=1, loop=True)[1] == 0
    assert _one([], path=((0.3, 0.0), (0.1, 0.0), (0.2, 0.0)), cursor=1, loop=True)[1] == 1
    # an open path stops at its last point and finishes there
    cmd, cur, rec = _one([], path=((0.1, 0.0), (0.2, 0.0)))
    assert cur == 1 and np.array_equal(cmd, A.STOP) and np.array_equal(rec, F([1, 0, 0, 0, 0, 0, 0, 1]))
    cmd, cur, rec = _one([], path=((0.1, 0.0), (2.0, 0.0)))
    assert cur == 1 and rec[7] == 0 and rec[1] == 3 and rec[3] == 2.0
    # P_k = 1: open -- it finishes inside reach; closed -- it steers for the one point for ever
    assert _one([], path=((0.5, 0.0),))[2][7] == 1 and _one([], path=((3.0, 0.0),))[2][7] == 0
    cmd, cur, rec = _one([], path=((0.5, 0.0),), loop=True)
    assert cur == 0 and rec[7] == 0 and rec[1] == 0 and cmd[3] == 2
    # an absent vehicle: stopped, the cursor left alone, the record zeros
    sc = AC.street([((0.0, 0.0), 0.0, (1.0, 0.0))])
    sc["dynamic_obstacles"][0] = (np.full(2, np.inf), sc["dynamic_obstacles"][0][1])
    st, fl = A.pack_settings(IO1, **EDGE)
    cmds, cur, rec = A.autopilot_scene(sc, None, [np.array([[0.1, 0.0], [5.0, 0.0]])], st, fl, np.array([1]), 0.05)
    assert np.array_equal(cmds[0], A.STOP) and cur[0] == 1 and not rec.any()


def test_the_turn():
    cmax, smax = F(np.cos(0.05)), F(np.sin(0.05))
    # inside the limit the commanded turn carries h onto g, up to the rounding bound of the unicycle's one normalisation
    for ang in (0.0, 0.01, -0.03, 0.049):
        cmd, _, _ = _one([], path=((50.0 * np.cos(ang), 50.0 * np.sin(ang)),), vel=(0.0, 0.0))
        h2, _ = scenarios.drive_command(2, cmd[:3], (1.0, 0.0))
        g = np.array([np.cos(ang), np.sin(ang)])
        assert np.hypot(*(h2.astype(np.float64) - g)) <= 50.0 * D.U * 4 + D.E_H + 3 * D.U + np.hypot(*(np.float32(50.0 * g).astype(np.float64) / 50.0 - g))
        assert abs(float(h2[0]) ** 2 + float(h2[1]) ** 2 - 1.0) <= D.H2_BOUND
    # outside it is exactly (cos_max, +-sin_max); a target exactly behind turns left
    for tgt, sgn in (((0.0, 30.0), 1), ((0.0, -30.0), -1), ((-30.0, 0.0), 1), ((10.0, -10.0), -1), ((-30.0, -1e-3), -1)):
        cmd, _, _ = _one([], path=(tgt,))
        assert cmd[1] == cmax and cmd[2] == sgn * smax, tgt
    # standing on the waypoint of a closed path: g = h, no turn
    cmd, _, _ = _one([], path=((0.0, 0.0),), loop=True)
    assert cmd[1] == 1.0 and cmd[2] == 0.0


def test_free_acceleration_rises_to_v0_and_stays():
    st, fl = A.pack_settings(IO1, loop=True, **AC.CALM)                  # (a closed path of one far point: no end of path ahead)
    sc = AC.street([((0.0, 0.0), 0.0, (0.0, 0.0))])
    recs, _, _ = AC.run_twin(sc, [np.array([[500.0, 0.0]])], st, fl, 0.05, 300)
    s = recs[:, 0, 6].astype(np.float64)
    v0, over = float(st[0, 0]), AC.overshoot_bound(st[0], 0.05)
    assert (np.diff(s) >= -over).all() and (np.diff(s)[s[:-1] < v0 * (1 - 1e-3)] > 0).all()
    assert s.max() <= v0 + over and s[-1] >= v0 * (1 - 1e-3) and not recs[:, 0, 1].any()


def _stand(ticks=400, **kw):
    sc, paths = AC.standing_pedestrian()
    loop, ign = kw.pop("loop", False), kw.pop("ignore_walkers", False)
    st, fl = A.pack_settings(IO1, loop=loop, ignore_walkers=ign, **dict(AC.CALM, **kw))
    return (sc, st) + AC.run_twin(sc, paths[0], st, fl, 0.05, ticks)


def test_a_standing_pedestrian_stops_the_vehicle():
    """The vehicle stops short: the gap never falls below s0 minus the derived bound (s_e the speed at the first tick at or below s0;
    the float64 rule, closed over the same scheme, itself never gets there with these settings), and it bites: the same scene
    with the vehicle free-running at v0 (kind 0, no controller) passes through the pedestrian, clearance below the body radius."""
    sc, st, recs, _, ctrs = _stand()
    gap, s = recs[:, 0, 3].astype(np.float64), recs[:, 0, 6].astype(np.float64)
    assert (recs[:, 0, 1] == 1).all() and (recs[:, 0, 2] == 0).all()
    below = np.flatnonzero(gap <= st[0, 2])
    s_e = float(s[below[0]]) if len(below) else 0.0
    assert gap.min() >= st[0, 2] - AC.undershoot_bound(s_e, st[0], 0.05)
    assert s.max() > 0.9 * st[0, 0] and s[-1] <= AC.STOPPED * st[0, 0]   # it did drive, and it has stopped
    # the float64 restatement in closed loop (x' = x - dt s', the same semi-implicit order)
    g64, s64, low = 30.0 - 2.5 - 0.5, 0.0, np.inf
    for _ in range(400):
        _, s64 = A.idm_f64(s64, 0.0, g64, True, st[0], 0.05)
        g64 -= np.float64(F(0.05)) * s64
        low = min(low, g64)
    assert low >= float(st[0, 2]) and s64 <= AC.STOPPED * st[0, 0]
    assert abs(gap[-1] - low) <= 1e-3                                    # both came to rest at the same place
    # the other half: the same scene, the vehicle free-running at v0 (not driven: it keeps its velocity)
    sc2, _ = AC.standing_pedestrian()
    sc2["dynamic_vel"] = np.array([[float(st[0, 0]), 0.0]])
    ped, clear = sc2["loc"][0, :2], np.inf
    for _ in range(400):
        scenarios.drive_vehicles(sc2, 0, np.zeros(3, F), 0.05)
        clear = min(clear, float(np.min(np.hypot(*(sc2["dynamic_obstacles"][0][1] - ped).T))))
    assert clear < 0.3 and sc2["dynamic_obstacles"][0][0][0] > ped[0] + 10.0
    # ... and autopiloted with walkers ignored it does the same
    sc3, st3, recs3, _, ctrs3 = _stand(ignore_walkers=True, loop=True)
    assert ctrs3[-1, 0, 0] > ped[0] + 10.0 and not recs3[:, 0, 1].any()


def test_a_pedestrian_who_walks_out_of_the_corridor_lets_the_vehicle_go():
    sc, paths = AC.standing_pedestrian(ahead=20.0)
    st, fl = A.pack_settings(IO1, loop=True, **AC.CALM)

    def walk(sc, t):
        if t >= 250:                                                     # after the vehicle has stopped: 1.2 m/s across the road
            sc["loc"][0, 1] = F(sc["loc"][0, 1] + 0.06)
            sc["vel"][0, 1] = F(1.2)
    recs, _, ctrs = AC.run_twin(sc, paths[0], st, fl, 0.05, 400, walk)
    s = recs[:, 0, 6]
    assert s[249] <= 0.02 * st[0, 0] and recs[249, 0, 1] == 1
    gone = np.flatnonzero(recs[:, 0, 1] == 0)
    assert len(gone) and gone[0] > 250 and (recs[gone[0]:, 0, 1] == 0).all()
    up = s[gone[0]:].astype(np.float64)
    assert (np.diff(up) >= 0).all() and (np.diff(up)[up[:-1] < st[0, 0] * (1 - 1e-3)] > 0).all()
    assert s[-1] > 0.5 * st[0, 0] and ctrs[-1, 0, 0] > 20.0


def test_a_follower_settles_at_the_equilibrium_gap():
    """Behind a slower free vehicle (kind 0: it keeps its velocity) the gap stays positive and comes to the IDM's equilibrium gap for
    the leader's speed.  The discrete map has the continuous model's fixed point (a = 0), so what is left after 400 ticks is the
    transient; the tolerance is one tick of travel, dt u_lead -- the resolution at which a gap is known between two ticks."""
    u_lead, dt = 1.5, 0.05
    sc = AC.street([((0.0, 0.0), 0.0, (0.0, 0.0)), ((25.0, 0.0), 0.0, (u_lead, 0.0))])
    st, fl = A.pack_settings(np.array([0, 2]), **AC.CALM)
    recs, _, _ = AC.run_twin(sc, [np.array([[2000.0, 0.0]]), None], st, fl, dt, 400)
    gap, s = recs[:, 0, 3].astype(np.float64), recs[:, 0, 6].astype(np.float64)
    assert (recs[:, 0, 1] == 2).all() and (recs[:, 0, 2] == 1).all() and (recs[:, 0, 4] == F(u_lead)).all()
    g_eq = A.equilibrium_gap(u_lead, st[0])
    assert gap.min() > 0 and abs(gap[-1] - g_eq) <= dt * u_lead and abs(s[-1] - u_lead) <= dt * u_lead
    g64, s64 = float(gap[0]), 0.0                                        # idm_f64 itself shows it
    for _ in range(400):
        _, s64 = A.idm_f64(s64, u_lead, g64, True, st[0], dt)
        g64 += np.float64(F(dt)) * (u_lead - s64)
    assert abs(g64 - g_eq) <= dt * u_lead and abs(gap[-1] - g64) <= dt * u_lead


def test_a_closed_path_is_driven_round():
    sc, paths = AC.closed_path()
    st, fl = A.pack_settings(IO1, loop=True, **dict(AC.CALM, v0=8.0))
    recs, curs, ctrs = AC.run_twin(sc, paths[0], st, fl, 0.05, 400)
    c = curs[:, 0]
    steps = np.mod(np.diff(c), 8)
    assert set(steps) <= {0, 1}                                          # every point in order, none skipped
    assert int(steps.sum()) >= 16                                        # two laps inside the budget
    assert np.max(np.abs(np.hypot(*ctrs[100:, 0].T) - 12.0)) < 3.0       # and it stays near its octagon


def test_packing_refuses_what_the_library_refuses():
    io = np.array([0, 2, 2, 3])
    off, px, py = A.pack_paths([[np.zeros((2, 2)), None], [], [np.ones((3, 2))]], io)
    assert off.tolist() == [0, 2, 2, 5] and px.dtype == np.float32 and len(px) == 5
    st, fl = A.pack_settings(io, v0=[[4.0, 5.0], 1.0, 6.0], loop=[True, False, True], ignore_walkers=np.array([0, 1, 0], bool), max_turn=0.1)
    assert st[:, 0].tolist() == [4.0, 5.0, 6.0] and fl.tolist() == [1, 3, 1]    # (a list is per scene, an ndarray (M,) per vehicle)
    assert st[0, 11] == F(np.cos(0.1)) and st[0, 12] == F(np.sin(0.1)) and st[0, 1] == F(A.DEFAULTS["T"])
    for bad in (dict(v0=0.0), dict(T=-1.0), dict(s0=0.0), dict(acc=np.inf), dict(dec=0.0), dict(brake=1.0, dec=2.0), dict(half_width=-1.0),
                dict(front=np.nan), dict(look=0.0), dict(reach=0.0), dict(reach=3e38), dict(ped_margin=-0.1), dict(max_turn=-0.1),
                dict(max_turn=np.pi / 2), dict(loop=2), dict(speed=1.0), dict(v0=[1.0, 2.0])):
        with pytest.raises(ValueError):
            A.pack_settings(io, **bad)
    for bad in ([[None]], [[None, None], [], [np.zeros(3)]], [[None, None], [], [np.full((1, 2), np.nan)]],
                [[None, None], [], [np.zeros((A.MAX_POINTS + 1, 2))]], [[None], [], [None]]):
        with pytest.raises(ValueError):
            A.pack_paths(bad, io)


def test_header_binding_and_symbols_agree():
    names = ("sfm_batch_set_vehicle_autopilot", "sfm_batch_download_vehicle_autopilot", "sfm_batch_vehicle_autopilot_launches")
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    for n in names:
        m = re.search(r"^int " + n + r"\(([^;]*)\);", header, re.M | re.S)
        assert m, n
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[n][1]), n
        assert n in _lib.UNBUMPED and _lib.SINCE[n] == _lib.ABI_VERSION
    for macro, v in (("SFM_BATCH_AUTOPILOT_SETTINGS", A.N_SETTINGS), ("SFM_BATCH_MAX_AUTOPILOT_POINTS", A.MAX_POINTS),
                     ("SFM_AUTOPILOT_LOOP", A.FLAG_LOOP), ("SFM_AUTOPILOT_IGNORE_WALKERS", A.FLAG_IGNORE_WALKERS)):
        assert re.search(rf"#define {macro} {v}\b", header), macro
    assert re.search(r"#define SFM_AUTOPILOT_GAP_FLOOR 0\.01f", header) and A.GAP_FLOOR == F(0.01)
    assert "sfm_batch_vehicle_autopilot_kernel" in open(os.path.join(CSRC, "resource_usage.txt")).read()
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        for n in names:
            assert re.search(rf"\bT {n}\b", out), n


def _example():
    import importlib.util
    spec = importlib.util.spec_from_file_location("batch_traffic_loop", os.path.join(ROOT, "examples", "batch_traffic_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_example_imports_without_a_gpu_and_its_circuits_pack():
    ex = _example()
    scenes = ex.make_scenes(3)
    paths = ex.circuits(scenes)
    io = np.concatenate(([0], np.cumsum([len(sc["dynamic_obstacles"]) for sc in scenes]))).astype(np.int32)
    off, px, py = A.pack_paths(paths, io)
    st, fl = A.pack_settings(io, loop=True, **ex.TRAFFIC)
    assert io[-1] > 0 and off[-1] == 4 * io[-1] and (fl == A.FLAG_LOOP).all() and st.shape == (io[-1], A.N_SETTINGS)
