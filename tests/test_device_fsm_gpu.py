"""SURVEY.md section 8f rows 1 and 3 on the GPU: pedestrian modes, waypoint queues, gap acceptance and despawn
inside sfm_run, against the host loop of the reference (its order, run_simulation.py:77-132 +
pedestrian_simulation.py:57-83) built from the host-side mirror classes and the float64 oracle.  The host
state is re-synchronised to the device's fp32 state every tick, so each tick's decisions are compared from
identical inputs; decisions within fp32 noise of their threshold are excluded.  The gap-acceptance decisions the device is
held to are the oracle's (oracle.sfm_oracle.gap_accepted); that oracle, and the device directly, are held to decisions of the reference's
own check_traffic in tests/test_traffic_golden.py and tests/test_gap_acceptance_gpu.py (what stays assumed there: a stand-in's definition
of shapely's segment intersection / distance)."""
import numpy as np
import pytest

from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd.check_traffic import check_traffic
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.engine import SfmEngine
from carla_social_force_model_amd.ped_mode_manager import PedMode, PedModeManager
from oracle import c_oracle
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu
DT, THR = 0.05, 2.0


def _park(pid):
    return np.array([np.float32(3.0e15) + np.float32(1.0e12) * np.float32(pid + 1), np.float32(-3.0e15)], dtype=np.float64)


@pytest.mark.parametrize("n", [160, 9000])
def test_modes_queues_gap_acceptance_and_despawn(n, monkeypatch):
    monkeypatch.setenv("SFM_RESORT_EVERY", "3")            # rows are re-sorted on the device during the run (n = 9000)
    rng = np.random.default_rng(n)
    sc = scenarios.make_scenario(n, 4000 + n, n_borders=6, n_dynamic=6, border_len=(5.0, 20.0))
    cfg = default_sfm_config()
    prm = O.OracleParams.from_config(cfg)
    ticks = 150 if n < 1000 else 8
    # mode objects: a few idle at t = 0 (wake up after 5 s), some who cross without looking
    fsm = []
    for i in range(n):
        m = PedModeManager(f"ped_{i}", float(sc.target_speed[i]), PedMode.WALKING_SIDEWALK, 1.5, -1.0 if i % 5 == 0 else 1.0)
        if i % 11 == 3:
            m.set_mode(PedMode.IDLE)
        fsm.append(m)
    # waypoint_dict: three more waypoints each, a few metres apart, every other leg crosses a road
    queues = []
    for i in range(n):
        p = sc.waypoint[i, :2].copy()
        lst = []
        for k in range(3):
            p = scenarios._f32(p + rng.uniform(-4.0, 4.0, 2))
            lst.append((np.array([p[0], p[1], 0.0]), bool((i + k) % 2)))
        queues.append(lst)
    sc.waypoint[:, :2] = scenarios._f32(sc.loc[:, :2] + rng.uniform(-3.0, 3.0, (n, 2)))   # first waypoints close by
    ext = sc.dynamic_extent

    eng = SfmEngine(cfg, DT)
    try:
        eng.set_borders(sc.borders, sc.border_centers, sc.border_lengths)
        eng.set_dynamic_boxes([c for c, _ in sc.dynamic_obstacles], sc.dynamic_yaw, ext, sc.dynamic_vel)
        eng.upload_state(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, None)
        eng.set_waypoint_stream(0, 0.0, THR)
        eng.set_mode_fsm(fsm, queues, despawn_on_arrival=True, sim_time0=0.0, first_vehicle_extent=ext[0])

        loc, vel, wp = sc.loc.copy(), sc.vel.copy(), sc.waypoint.copy()
        tspeed = sc.target_speed.copy()
        alive = np.ones(n, bool)
        remaining = [list(q) for q in queues]
        events = dict(idle_wake=0, checking=0, crossing=0, road_to_sidewalk=0, despawn=0, popped=0)
        for k in range(ticks):
            t = k * DT
            geom = O.Geometry(sc.borders, sc.border_centers, sc.border_lengths, [], sc.dynamic_obstacles, sc.dynamic_vel)
            # ---- host tick (reference order) ----
            for i in range(n):
                if alive[i]:
                    tspeed[i] = fsm[i].target_speed                       # apply_current_mode
            unsure = np.zeros(n, bool)
            for i in range(n):
                if not alive[i]:
                    continue
                was = fsm[i].current_mode
                fsm[i].tick(t)
                events["idle_wake"] += was == PedMode.IDLE and fsm[i].current_mode == PedMode.WALKING_SIDEWALK
                if fsm[i].current_mode == PedMode.CHECKING_TRAFFIC:
                    # the expected decision comes from the ORACLE's float64 restatement of check_traffic.py:7-61 (round-2 verdict
                    # item 9), not from the product's own host function -- which must agree with it on the same inputs
                    go = O.gap_accepted(loc[i], wp[i], fsm[i].crossing_speed, fsm[i].crossing_safety_margin,
                                        [c for c, _ in sc.dynamic_obstacles], sc.dynamic_vel, ext)
                    rec = {"loc": loc[i], "next_waypoint": wp[i], "mode": fsm[i]}
                    assert check_traffic(rec, sc.dynamic_obstacles, list(sc.dynamic_vel), list(ext)) == go
                    if go:
                        fsm[i].set_mode(PedMode.CROSSING_ROAD)
                        events["crossing"] += 1
            crossing = np.array([alive[i] and fsm[i].current_mode in (PedMode.CROSSING_ROAD, PedMode.ROAD_TO_SIDEWALK) for i in range(n)])
            if n < 1000:
                with np.errstate(all="ignore"):
                    _, F, _ = O.tick_forces(loc, vel, wp, np.where(alive, tspeed, 0.0), sc.radius, crossing, geom, prm)
                v_new = O.new_velocities(vel, F, np.where(alive, tspeed, 0.0), DT)
            else:                                              # the C port of the oracle for the large crowd
                _, _, v_new, _, _ = c_oracle.tick(loc, vel, wp, np.where(alive, tspeed, 0.0), sc.radius, crossing, geom, prm, DT)
            dist = np.linalg.norm(wp[:, :2] - loc[:, :2], axis=1)
            unsure |= np.abs(dist - THR) < 1e-4
            for i in np.nonzero((dist < THR) & alive)[0]:
                if remaining[i]:
                    nxt, cross = remaining[i].pop(0)
                    wp[i] = nxt
                    before = fsm[i].current_mode
                    fsm[i].set_mode(PedMode.CROSSING_ROAD if cross else PedMode.WALKING_SIDEWALK)
                    events["popped"] += 1
                    events["checking"] += fsm[i].current_mode == PedMode.CHECKING_TRAFFIC and before != PedMode.CHECKING_TRAFFIC
                    events["road_to_sidewalk"] += fsm[i].current_mode == PedMode.ROAD_TO_SIDEWALK
                else:
                    alive[i] = False
                    events["despawn"] += 1
            new_loc = loc + DT * v_new
            for i in np.nonzero(~alive)[0]:
                new_loc[i, :2] = _park(i); v_new[i] = 0.0
            # ---- device tick ----
            eng.run(1)
            dloc, dvel, dwp = eng.state()
            dmode, dtarget, dcursor = eng.modes()
            ok = ~unsure
            hmode = np.array([int(fsm[i].current_mode) if alive[i] else 255 for i in range(n)])
            assert np.array_equal(dmode[ok], hmode[ok]), f"modes differ at tick {k}: {np.nonzero(dmode != hmode)[0][:5]}"
            assert np.array_equal(dcursor[ok], np.array([3 - len(r) for r in remaining])[ok]), f"cursors at tick {k}"
            htarget = np.array([fsm[i].target_speed if alive[i] else 0.0 for i in range(n)])
            assert np.allclose(dtarget[ok], htarget[ok], rtol=1e-6), f"mode target speeds at tick {k}"
            assert np.allclose(dwp[ok], wp[ok, :2], atol=1e-4), f"waypoints at tick {k}"
            live = alive & ok
            assert np.max(np.abs(dvel[live] - v_new[live])) <= 2e-4 * max(1.0, np.max(np.abs(v_new[live]))), f"v' at tick {k}"
            assert np.allclose(dloc[~alive & ok, :2], new_loc[~alive & ok, :2]), "parked ghosts"
            # re-sync the host to the device's fp32 state (FSM objects keep evolving on the host)
            for i in np.nonzero(unsure)[0]:                   # borderline arrival: adopt the device's decision
                cur = int(dcursor[i])
                while 3 - len(remaining[i]) < cur:
                    nxt, cross = remaining[i].pop(0)
                    fsm[i].set_mode(PedMode.CROSSING_ROAD if cross else PedMode.WALKING_SIDEWALK)
                if dmode[i] == 255:
                    alive[i] = False
            loc, vel = dloc, dvel
            wp = np.concatenate([dwp, np.zeros((n, 1))], axis=1)
            scenarios.advance_dynamic(sc, DT)
        if n < 1000:                                           # the run actually exercised every branch
            assert events["popped"] > n and events["checking"] > 10 and events["crossing"] > 10
            assert events["road_to_sidewalk"] > 5 and events["idle_wake"] > 5 and events["despawn"] > 5, events
    finally:
        eng.close()
