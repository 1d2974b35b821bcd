"""GPU tests of the batch's pedestrian modes (sfm_batch_set_mode_fsm, sfm_batch_download_modes; SfmBatch.set_modes / modes /
clocks): every tick of every scene against the reference's host loop (PedModeManager mirrors, the float64 oracle's gap acceptance
and forces, the host twin of the vehicles), agreement with a handle's set_mode_fsm, scene independence, the run forms, refused
input and a batch at size.  Run on the MI355X box with  python -m pytest tests -m gpu."""
from types import SimpleNamespace

import numpy as np
import pytest

import _parity as P
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import MODE_KEYS, SfmBatch, mode_scene_arrays, pack_modes
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.engine import SfmEngine
from carla_social_force_model_amd.ped_mode_manager import PedMode
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

ALL = scenarios.ALL_FORCES
GONE = 255


def _park(i):
    return np.array([np.float32(3.0e15) + np.float32(1.0e12) * np.float32(i + 1), np.float32(-3.0e15)], dtype=np.float64)


def _scene(n, seed, dynamic, z_spread=0.0, borders=3):
    sc = vars(scenarios.make_scenario(n, seed, n_borders=borders, n_static=1, n_dynamic=dynamic, z_spread=z_spread,
                                      border_len=(3.0, 15.0)))
    rng = np.random.default_rng(seed + 17)
    sc["radius"] = np.float32(rng.uniform(0.2, 0.45, n)).astype(np.float64)
    sc["dynamic_vel"] = np.float32(sc["dynamic_vel"] * 0.1).astype(np.float64)     # slow: the plain 1e-5 bound on v' holds
    if dynamic and n:                                                               # vehicles inside the crowd
        c = np.float32(sc["loc"][rng.integers(0, n, dynamic), :2] + rng.uniform(-1.0, 1.0, (dynamic, 2))).astype(np.float64)
        sc["dynamic_obstacles"] = [(c[k], scenarios.place_ring_f32(c[k], sc["dynamic_yaw"][k],
                                                                   scenarios.ring_local_offsets(*sc["dynamic_extent"][k])))
                                   for k in range(dynamic)]
    plan, ms = scenarios.make_mode_plan(sc, seed + 5)
    return sc, plan, ms


def _config(k, forces=ALL):
    cfg = default_sfm_config(forces)
    cfg["pedestrian_force"].update({"A": 3.0 + 0.5 * k, "lambda": 1.5 + 0.1 * k})
    cfg["goal_force"] = {"tau": 0.4 + 0.05 * k}
    cfg["use_ped_radius"] = bool(k % 2)
    return cfg


def _advance(sc, dt):
    ns = SimpleNamespace(**sc)
    scenarios.advance_dynamic(ns, dt)
    sc["dynamic_obstacles"] = ns.dynamic_obstacles


def _batch(scenes, plans, cfgs, dts, despawn=True, t0=0.0, thr=2.0, planar=None):
    b = SfmBatch(cfgs, dts)
    b.upload(scenes, planar=planar, device_vehicles=True)
    b.set_modes(plans, despawn_on_arrival=despawn, sim_time0=t0, arrive_thresholds=thr, scenes=scenes)
    return b


def _everything(b):
    """State, waypoints, modes, targets, cursors of every scene, and the clocks."""
    return [(loc, vel, wp, m, t, c) for (loc, vel), (wp, _), (m, t, c) in zip(b.state(), b.waypoints(), b.modes())], b.clocks()


def _assert_same(xs, ys, what):
    (a, ca), (b, cb) = xs, ys
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for q, (u, v) in enumerate(zip(x, y)):
            assert u.shape == v.shape and np.array_equal(u, v), f"{what}: scene {k}, field {q}"
    assert np.array_equal(ca, cb), f"{what}: clocks"


class _Host:
    """The reference's host loop for one scene (test_device_fsm_gpu.py's order), re-synchronised to the device every tick."""

    def __init__(self, sc, plan, ms, cfg, dt, thr, despawn):
        self.sc, self.ms, self.dt, self.thr, self.despawn = sc, ms, dt, thr, despawn
        self.prm = O.OracleParams.from_config(cfg)
        self.n = len(ms)
        self.alive = np.ones(self.n, bool)
        self.remaining = [list(q) for q in plan["queues"]]
        self.qlen = np.array([len(q) for q in plan["queues"]])

    def tick(self, loc, vel, wp2, vehicles, t, ev):
        n, ms, alive = self.n, self.ms, self.alive
        wp = np.zeros((n, 3))
        wp[:, :2] = wp2
        tspeed = np.array([ms[i].target_speed if alive[i] else 0.0 for i in range(n)], dtype=np.float64)
        centres = [c for c, _ in vehicles]
        for i in range(n):
            if not alive[i]:
                continue
            was = ms[i].current_mode
            ms[i].tick(t)
            ev["idle_wake"] += was == PedMode.IDLE and ms[i].current_mode == PedMode.WALKING_SIDEWALK
            if ms[i].current_mode == PedMode.CHECKING_TRAFFIC:
                go = not centres or O.gap_accepted(loc[i], wp[i], ms[i].crossing_speed, ms[i].crossing_safety_margin, centres,
                                                   self.sc["dynamic_vel"], self.sc["dynamic_extent"])
                ev["waiting"] += not go
                if go:
                    ms[i].set_mode(PedMode.CROSSING_ROAD)
                    ev["crossing"] += 1
        crossing = np.array([alive[i] and ms[i].current_mode in (PedMode.CROSSING_ROAD, PedMode.ROAD_TO_SIDEWALK) for i in range(n)])
        sc = self.sc
        geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"],
                          dynamic_obstacles=vehicles, dynamic_vel=sc["dynamic_vel"])
        diag = {}
        with np.errstate(all="ignore"):
            _, F, _ = O.tick_forces(loc, vel, wp, tspeed, sc["radius"], crossing, geom, self.prm, theta_tol=P.THETA_TOL,
                                    tie_rel=P.TIE_REL, diag=diag)
            v_new = O.new_velocities(vel, F, tspeed, self.dt)
        dist = np.linalg.norm(wp[:, :2] - loc[:, :2], axis=1)
        unsure = np.abs(dist - self.thr) < 1e-4
        for i in np.nonzero((dist < self.thr) & alive)[0]:
            if self.remaining[i]:
                nxt, cross = self.remaining[i].pop(0)
                wp[i, :2] = np.asarray(nxt, dtype=np.float64)[:2]
                before = ms[i].current_mode
                ms[i].set_mode(PedMode.CROSSING_ROAD if cross else PedMode.WALKING_SIDEWALK)
                ev["popped"] += 1
                ev["checking"] += ms[i].current_mode == PedMode.CHECKING_TRAFFIC and before != PedMode.CHECKING_TRAFFIC
                ev["road_to_sidewalk"] += ms[i].current_mode == PedMode.ROAD_TO_SIDEWALK
            elif self.despawn:
                alive[i] = False
                ev["despawn"] += 1
        return v_new, wp[:, :2], unsure, diag["total"]

    def check(self, k, t, dloc, dvel, dwp, dmode, dtarget, dcursor, v_new, wp, unsure, diag):
        n, ms, alive = self.n, self.ms, self.alive
        ok = ~unsure
        hmode = np.array([int(ms[i].current_mode) if alive[i] else GONE for i in range(n)])
        assert np.array_equal(dmode[ok], hmode[ok]), f"scene {k} tick {t}: modes differ at {np.nonzero(dmode != hmode)[0][:5]}"
        hcur = self.qlen - np.array([len(r) for r in self.remaining], dtype=np.int64)
        assert np.array_equal(dcursor[ok], hcur[ok]), f"scene {k} tick {t}: cursors"
        htarget = np.array([ms[i].target_speed if alive[i] else 0.0 for i in range(n)])
        assert np.allclose(dtarget[ok], htarget[ok], rtol=1e-6, atol=0), f"scene {k} tick {t}: mode target speeds"
        assert np.allclose(dwp[ok], wp[ok], atol=1e-4, rtol=0), f"scene {k} tick {t}: waypoints"
        # v': 1e-5 plus, as test_batch_gpu.py allows for scenes with vehicles, the conditioning term of a force that is a small sum
        # of larger terms (a pedestrian pushed by the crowd against its own drive) -- needed by a few rows at most
        expo, summed = diag
        live = alive & ok
        needed = P.check_velocity_conditioned(dvel[live], v_new[live], expo[live], summed[live], self.dt)
        assert needed <= max(2, n // 50), f"scene {k} tick {t}: {needed} rows needed the conditioning term"
        for i in np.nonzero(~alive & ok)[0]:
            assert np.array_equal(dloc[i, :2], _park(i)) and not dvel[i].any(), f"scene {k} tick {t}: ghost {i}"
        # re-synchronise the host's mode objects to the device's borderline arrivals
        for i in np.nonzero(unsure)[0]:
            while self.qlen[i] - len(self.remaining[i]) < dcursor[i]:
                nxt, cross = self.remaining[i].pop(0)
                self.ms[i].set_mode(PedMode.CROSSING_ROAD if cross else PedMode.WALKING_SIDEWALK)
            if dmode[i] == GONE:
                alive[i] = False


def test_every_tick_matches_the_host_loop():
    """8 scenes of 0, 1, 2, 64, 65, 200, 300 and 1024 pedestrians (every slice shape), their own step lengths, A, borders, moving
    vehicles and despawn switch; 150 ticks (the 1024-pedestrian scene is compared on the first 12): modes, cursors, despawns, mode
    targets, waypoints, parked ghosts and v' of every scene against the reference's host loop on the device's state."""
    sizes = (0, 1, 2, 64, 65, 200, 300, 1024)
    dts = [0.05, 0.04, 0.05, 0.03, 0.05, 0.04, 0.05, 0.05]
    despawn = [1, 0, 1, 1, 0, 1, 1, 0]
    t0 = [4.0, 3.0, 4.5, 3.5, 4.0, 3.0, 2.5, 0.0]           # the IDLE pedestrians wake up inside the run
    thr = [2.0, 2.5, 2.0, 2.0, 1.5, 2.0, 2.5, 2.0]
    made = [_scene(n, 900 + k, 4 if n else 2) for k, n in enumerate(sizes)]
    scenes = [m[0] for m in made]
    cfgs = [_config(k) for k in range(len(sizes))]
    b = _batch(scenes, [m[1] for m in made], cfgs, dts, despawn, t0, thr)
    hosts = [_Host(sc, plan, ms, cfg, dt, th, d) for (sc, plan, ms), cfg, dt, th, d in zip(made, cfgs, dts, thr, despawn)]
    ev = dict(idle_wake=0, waiting=0, checking=0, crossing=0, road_to_sidewalk=0, despawn=0, popped=0)
    clock = np.float32(t0)
    try:
        for t in range(150):
            assert np.array_equal(b.clocks(), clock), f"clocks before tick {t}"
            state, wps, veh = b.state(), b.waypoints(), b.dynamic_obstacles()
            expect = {}
            for k, h in enumerate(hosts):
                if h.n == 0 or (h.n > 500 and t >= 12):
                    continue
                loc, vel = state[k]
                expect[k] = h.tick(loc, vel, wps[k][0].astype(np.float64), veh[k], float(clock[k]), ev)
            b.run(1)
            clock = (clock + np.float32(dts)).astype(np.float32)
            after, wps2, modes = b.state(), b.waypoints(), b.modes()
            for k, (v_new, wp, unsure, diag) in expect.items():
                hosts[k].check(k, t, after[k][0], after[k][1], wps2[k][0].astype(np.float64), *modes[k], v_new, wp, unsure, diag)
            for sc, dt in zip(scenes, dts):
                _advance(sc, dt)
        assert np.array_equal(b.clocks(), clock)
        assert ev["popped"] > 300 and ev["checking"] > 20 and ev["crossing"] > 20 and ev["waiting"] > 5, ev
        assert ev["road_to_sidewalk"] > 10 and ev["idle_wake"] > 10 and ev["despawn"] > 10, ev
    finally:
        b.close()


def test_agrees_with_the_handle():
    """A one-scene batch and SfmEngine.set_mode_fsm, the handle handed the batch's state, modes, targets, remaining queues and
    clock every tick: modes, mode targets and cursors bitwise equal, v' within 1e-5; the batch's clock is the handle's float
    sum sim_time0 + dt + dt + ... bit for bit."""
    sc, plan, ms = _scene(64, 515, 4)
    cfg, dt = _config(0), 0.05
    b = _batch([sc], [plan], [cfg], [dt], despawn=False, t0=4.0)
    eng = SfmEngine(cfg, dt)
    queues = [list(q) for q in plan["queues"]]
    pm = pack_modes([plan], np.array([0, 64], np.int32))
    clock = np.float32(4.0)
    try:
        eng.set_borders(sc["borders"], sc["border_centers"], sc["border_lengths"])
        eng.set_static_obstacles(sc["static_obstacles"])
        eng.set_dynamic_boxes([c for c, _ in sc["dynamic_obstacles"]], sc["dynamic_yaw"], sc["dynamic_extent"], sc["dynamic_vel"])
        checking = 0
        for t in range(60):
            (loc, vel), = b.state()
            wp = np.zeros((64, 3))
            wp[:, :2] = b.waypoints()[0][0]
            (m0, t0, c0), = b.modes()
            assert b.clocks()[0] == clock
            eng.upload_state(loc, vel, wp, sc["target_speed"], sc["radius"], None)
            mirrors = [SimpleNamespace(current_mode=int(m0[i]), target_speed=float(t0[i]), initial_target_speed=float(pm["initial_speed"][i]),
                                       crossing_speed=float(pm["crossing_speed"][i]), crossing_safety_margin=float(pm["safety_margin"][i]),
                                       next_mode_time=float(pm["next_mode_time"][i])) for i in range(64)]
            eng.set_mode_fsm(mirrors, [queues[i][c0[i]:] for i in range(64)], despawn_on_arrival=False, sim_time0=float(clock),
                             first_vehicle_extent=sc["dynamic_extent"][0])
            geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"],
                              dynamic_obstacles=b.dynamic_obstacles()[0], dynamic_vel=sc["dynamic_vel"])
            diag = {}
            ts = np.asarray(t0, dtype=np.float64)
            with np.errstate(all="ignore"):
                O.tick_forces(loc, vel, wp, ts, sc["radius"], np.zeros(64, bool), geom, O.OracleParams.from_config(cfg),
                              theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
            b.run(1)
            eng.run(1)
            clock = np.float32(clock + np.float32(dt))
            (m1, t1, c1), = b.modes()
            hm, ht, hc = eng.modes()
            assert np.array_equal(m1, hm), f"tick {t}: modes"
            assert np.array_equal(t1.view(np.uint32), ht.view(np.uint32)), f"tick {t}: targets"
            assert np.array_equal(c1, c0 + hc), f"tick {t}: cursors"
            P.check_velocity(b.state()[0][1], eng.state()[1], diag["total"][0], dt)
            checking += int((m1 == int(PedMode.CHECKING_TRAFFIC)).sum())
        assert b.clocks()[0] == clock
        assert checking > 0
    finally:
        b.close()
        eng.close()


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_scene_is_independent_of_the_batch(z_spread):
    """A scene with modes and moving vehicles, alone and at positions 0, 3 and 7 of a batch of 8 mixed scenes, over 100 ticks:
    state, waypoints, modes, targets, cursors and clock bitwise identical."""
    target = _scene(65, 77, 4, z_spread)
    tcfg, tdt = _config(3), 0.04
    others = [_scene(n, 1000 + k, m, z_spread) for k, (n, m) in enumerate(((30, 2), (0, 1), (130, 0), (1, 5), (250, 3)))]
    made = [target] + others[:2] + [target] + others[2:] + [target]
    cfgs = [tcfg] + [_config(k) for k in range(2)] + [tcfg] + [_config(k) for k in range(2, 5)] + [tcfg]
    dts = [tdt, 0.05, 0.02, tdt, 0.05, 0.03, 0.05, tdt]
    t0 = [1.0, 0.0, 2.0, 1.0, 0.5, 4.0, 3.0, 1.0]
    planar = z_spread == 0.0
    alone = SfmBatch([tcfg], [tdt])
    mixed = SfmBatch(cfgs, dts)
    try:
        alone.upload([target[0]], planar=planar, device_vehicles=True)
        alone.set_modes([target[1]], sim_time0=1.0, scenes=[target[0]])
        mixed.upload([m[0] for m in made], planar=planar, device_vehicles=True)
        mixed.set_modes([m[1] for m in made], despawn_on_arrival=[1, 0, 1, 1, 0, 1, 0, 1], sim_time0=t0,
                        scenes=[m[0] for m in made])
        alone.run(40)
        mixed.run(40)
        alone.tick(integrate=True)
        mixed.tick(integrate=True)
        alone.tick()
        mixed.tick()
        alone.run(58)
        mixed.run(58)
        (a, ca), (m, cm) = _everything(alone), _everything(mixed)
        for pos in (0, 3, 7):
            _assert_same((a, ca), (m[pos:pos + 1], cm[pos:pos + 1]), f"alone vs position {pos}")
        assert (a[0][5] > 0).any() and (a[0][3] != int(PedMode.WALKING_SIDEWALK)).any()
    finally:
        alone.close()
        mixed.close()


def test_run_forms_agree():
    """run(K) == K x tick(integrate=True) bit for bit with modes and moving vehicles; run_recorded frames == step-wise downloads."""
    made = [_scene(64, 41, 4), _scene(17, 42, 1), _scene(0, 43, 2), _scene(120, 44, 3)]
    scenes, plans = [m[0] for m in made], [m[1] for m in made]
    cfgs = [_config(k) for k in range(4)]
    dts = [0.05, 0.04, 0.02, 0.05]
    A, B_, Cb, D = (_batch(scenes, plans, cfgs, dts, t0=4.0) for _ in range(4))
    try:
        A.run(30)
        for _ in range(30):
            B_.tick(integrate=True)
        _assert_same(_everything(A), _everything(B_), "run(30) vs 30 x tick")
        frames, idx, _ = Cb.run_recorded(29, stride=4)
        assert list(idx) == list(range(0, 29, 4))
        want = [[] for _ in scenes]
        for k in idx:
            for s, (loc, vel) in enumerate(D.state()):
                want[s].append(np.float32(np.concatenate([loc[:, :2], vel[:, :2]], axis=1)))
            D.run(min(4, 29 - k))
        for s, sc in enumerate(scenes):
            assert np.array_equal(frames[s], np.stack(want[s]).reshape(len(idx), len(sc["loc"]), 4)), f"scene {s}: frames"
        _assert_same(_everything(Cb), _everything(D), "run_recorded vs run")
    finally:
        for b in (A, B_, Cb, D):
            b.close()


def test_refusals_leave_the_batch_unchanged():
    """Every bad argument of sfm_batch_set_mode_fsm, sfm_batch_download_modes before modes, and SFM_TICK_REDRAW_WAYPOINTS while
    modes are set: SFM_ERR_INVALID / SFM_ERR_STATE with a message, the batch bitwise unchanged and stepping as a fresh one.  upload
    and mode = NULL switch the modes off (modes() refused, redraw=True works again)."""
    L = _lib.load()
    made = [_scene(20, 81, 2), _scene(10, 82, 3)]
    scenes, plans = [m[0] for m in made], [m[1] for m in made]
    cfgs, dts = [_config(0), _config(1)], [0.05, 0.04]
    empty = SfmBatch(cfgs, dts)
    b = _batch(scenes, plans, cfgs, dts)
    fresh = _batch(scenes, plans, cfgs, dts)
    try:
        pm = pack_modes(plans, b.scene_off, scenes)
        despawn, t0, thr = mode_scene_arrays(2)
        good = [pm["mode"]] + [pm[k] for k in MODE_KEYS[1:]] + [pm["wp_offsets"], pm["wp_x"], pm["wp_y"], pm["wp_crossing"],
                                                               despawn, t0, thr, pm["first_vehicle_extent"]]
        p = lambda a: None if a is None else a.ctypes.data

        def bad(i, a):
            args = list(good)
            args[i] = a
            return args

        assert L.sfm_batch_set_mode_fsm(empty._b, *(p(a) for a in good)) == -3           # SFM_ERR_STATE: no state
        assert "upload_state" in L.sfm_batch_last_error(empty._b).decode()
        assert L.sfm_batch_download_modes(empty._b, None, None, None, None) == -3
        off = pm["wp_offsets"]
        mode7 = pm["mode"].copy()
        mode7[3] = 7
        cases = [(bad(i, None), "NULL") for i in range(1, 7)]
        cases += [(bad(i, None), "NULL") for i in (10, 11, 12)]
        cases += [(bad(0, mode7), "0..4"),
                  (bad(6, (off + 1).astype(np.int32)), "[0] must be 0"),
                  (bad(6, np.concatenate([off[:3], off[2:3] - 1, off[4:]]).astype(np.int32)), "non-decreasing"),
                  (bad(7, None), "waypoint arrays are NULL"), (bad(8, None), "waypoint arrays are NULL"),
                  (bad(9, None), "waypoint arrays are NULL"),
                  (bad(12, np.float32([2.0, -1.0])), "arrive_threshold"), (bad(12, np.float32([np.inf, 2.0])), "arrive_threshold"),
                  (bad(12, np.float32([np.nan, 2.0])), "arrive_threshold"), (bad(11, np.float32([0.0, np.nan])), "sim_time0")]
        # (arguments: 0 mode, 1-5 target / initial / crossing speed, margin, next_mode_time, 6 wp_offsets, 7-9 wp_x / wp_y /
        #  wp_crossing, 10 despawn_on_arrival, 11 sim_time0, 12 arrive_threshold, 13 first_vehicle_extent)
        b.run(3)
        fresh.run(3)
        before = _everything(b)
        for k, (args, msg) in enumerate(cases):
            rc = L.sfm_batch_set_mode_fsm(b._b, *(p(a) for a in args))
            assert rc == -1, f"case {k}: {rc}"                                                # SFM_ERR_INVALID
            err = L.sfm_batch_last_error(b._b).decode()
            assert msg in err, f"case {k}: {err!r}"
        for call in (lambda: L.sfm_batch_tick(b._b, 3), lambda: L.sfm_batch_run(b._b, 2, 2)):
            assert call() == -1
            err = L.sfm_batch_last_error(b._b).decode()
            assert "SFM_TICK_INTEGRATE" in err and "queues" in err, err
        b.set_waypoint_streams(5, 10.0)
        with pytest.raises(_lib.SfmLibraryError, match="SFM_TICK_INTEGRATE"):
            b.run(2, redraw=True)
        with pytest.raises(_lib.SfmLibraryError, match="SFM_TICK_INTEGRATE"):
            b.run_recorded(2, redraw=True)
        _assert_same(_everything(b), before, "after the refused calls")
        b.run(5)
        fresh.run(5)
        _assert_same(_everything(b), _everything(fresh), "refused calls vs a fresh batch")

        b.upload(scenes, device_vehicles=True)                 # a new crowd: modes off
        with pytest.raises(_lib.SfmLibraryError, match="sfm_batch_set_mode_fsm"):
            b.modes()
        b.run(2, redraw=True)
        b.set_modes(plans)
        b.run(1)
        b.set_modes(None)                                      # mode = NULL: off
        with pytest.raises(_lib.SfmLibraryError, match="sfm_batch_set_mode_fsm"):
            b.clocks()
        b.run(2, redraw=True)
    finally:
        for x in (b, fresh, empty):
            x.close()


def test_at_size():
    """1024 scenes x 64 pedestrians, all five forces, 4 moving vehicles and modes each, 200 ticks: every scene finite, the ghosts
    parked, and the count of every mode per scene equal to a re-run of 8 of the scenes in batches of one."""
    B, T = 1024, 200
    made = [_scene(64, 5000 + k, 4, borders=2) for k in range(B)]
    scenes, plans = [m[0] for m in made], [m[1] for m in made]
    # (radii off: with them two pedestrians that overlap can meet a pedestrian force beyond fp32's range -- the reference's own
    #  1e56 in float64 -- which no fp32 kernel represents)
    cfgs = [_config(2 * (k % 2)) for k in range(B)]
    dts = [(0.05, 0.04, 0.02, 0.03)[k % 4] for k in range(B)]
    despawn = [k % 3 != 0 for k in range(B)]
    t0 = [float(k % 5) for k in range(B)]
    b = _batch(scenes, plans, cfgs, dts, despawn, t0)
    try:
        b.run(T)
        state, modes = b.state(), b.modes()
        totals = np.zeros(256, np.int64)
        for k, ((loc, vel), (m, _, _)) in enumerate(zip(state, modes)):
            assert np.isfinite(loc).all() and np.isfinite(vel).all(), f"scene {k}"
            gone = np.nonzero(m == GONE)[0]
            for i in gone:
                assert np.array_equal(loc[i, :2], _park(i)) and not vel[i].any(), f"scene {k} ghost {i}"
            totals += np.bincount(m, minlength=256)
        assert totals[GONE] > 100 and totals[int(PedMode.CHECKING_TRAFFIC)] + totals[int(PedMode.CROSSING_ROAD)] > 100, totals[:5]
        for k in (0, 1, 2, 3, 400, 511, 777, 1023):
            one = SfmBatch([cfgs[k]], [dts[k]])
            try:
                one.upload([scenes[k]], device_vehicles=True)
                one.set_modes([plans[k]], despawn_on_arrival=despawn[k], sim_time0=t0[k], scenes=[scenes[k]])
                one.run(T)
                (m1, _, _), = one.modes()
                assert np.array_equal(np.bincount(m1, minlength=256), np.bincount(modes[k][0], minlength=256)), f"scene {k}"
                assert np.array_equal(m1, modes[k][0]), f"scene {k}"
            finally:
                one.close()
    finally:
        b.close()
