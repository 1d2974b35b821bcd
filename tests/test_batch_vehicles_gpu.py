"""GPU tests of the batch's device-side vehicles (sfm_batch_set_dynamic_boxes, sfm_batch_download_dynamic_obstacles; SfmBatch.
set_dynamic_boxes / dynamic_obstacles, upload(device_vehicles=True)): the vehicles against the host twin bit for bit, the tick
against the oracle with the twin's geometry, the run forms against each other, batch invariance, agreement with the handle's
device-side vehicles, switching between boxes and rings, refused input, and a batch at size.
Run on the MI355X box with  python -m pytest tests -m gpu."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import _parity as P
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import SfmBatch, pack_boxes, pack_scenes
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.engine import SfmEngine
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

ALL = scenarios.ALL_FORCES
NO_DYN = ("acceleration_force", "pedestrian_force", "border_force", "static_obstacle_force")


def _scene(n, seed, dynamic, z_spread=0.0, borders=3, static=2, slow=True):
    sc = vars(scenarios.make_scenario(n, seed, n_borders=borders, n_static=static, n_dynamic=dynamic, z_spread=z_spread,
                                      border_len=(3.0, 15.0)))
    rng = np.random.default_rng(seed + 17)
    sc["radius"] = np.float32(rng.uniform(0.2, 0.45, n)).astype(np.float64)
    if slow:                # slow vehicles: the plain 1e-5 bound on v' holds (see _parity.check_velocity_conditioned)
        sc["dynamic_vel"] = np.float32(sc["dynamic_vel"] * 0.1).astype(np.float64)
    # vehicles start inside the crowd, so the dynamic-obstacle force acts
    if dynamic and n:
        c = np.float32(sc["loc"][rng.integers(0, n, dynamic), :2] + rng.uniform(-1.0, 1.0, (dynamic, 2))).astype(np.float64)
        sc["dynamic_obstacles"] = [(c[k], sc["dynamic_obstacles"][k][1]) for k in range(dynamic)]
    _restart_twin(sc)
    return sc


def _config(k, forces):
    cfg = default_sfm_config(forces)
    cfg["pedestrian_force"].update({"A": 3.0 + 0.5 * k, "lambda": 1.5 + 0.1 * k})
    cfg["goal_force"] = {"tau": 0.4 + 0.05 * k}
    cfg["use_ped_radius"] = bool(k % 2)
    return cfg


def _restart_twin(sc):
    """The scene's rings regenerated at its centres in the device's arithmetic (what set_dynamic_boxes leaves)."""
    sc["dynamic_obstacles"] = [(np.asarray(c, dtype=np.float64),
                                scenarios.place_ring_f32(c, sc["dynamic_yaw"][k], scenarios.ring_local_offsets(*sc["dynamic_extent"][k])))
                               for k, (c, _) in enumerate(sc["dynamic_obstacles"])]


def _advance(sc, dt):
    """The host twin: one integrating tick of the scene's vehicles (scenarios.advance_dynamic on the dict)."""
    ns = SimpleNamespace(**sc)
    scenarios.advance_dynamic(ns, dt)
    sc["dynamic_obstacles"] = ns.dynamic_obstacles


def _same_vehicles(dev, sc, what):
    assert len(dev) == len(sc["dynamic_obstacles"]), what
    for j, ((c_d, r_d), (c_h, r_h)) in enumerate(zip(dev, sc["dynamic_obstacles"])):
        assert np.array_equal(c_d, c_h), f"{what}: vehicle {j} centre"
        assert r_d.shape == r_h.shape and np.array_equal(r_d, r_h), f"{what}: vehicle {j} ring"


def _batch(scenes, cfgs, dts, planar=None):
    b = SfmBatch(cfgs, dts)
    b.upload(scenes, planar=planar, device_vehicles=True)
    return b


def _everything(b):
    return [(loc, vel, [c for c, _ in veh], [r for _, r in veh]) for (loc, vel), veh in zip(b.state(), b.dynamic_obstacles())]


def _assert_same(xs, ys, what):
    assert len(xs) == len(ys)
    for k, (x, y) in enumerate(zip(xs, ys)):
        for q, (u, v) in enumerate(zip(x, y)):
            if isinstance(u, list):
                assert len(u) == len(v) and all(np.array_equal(a, c) for a, c in zip(u, v)), f"{what}: scene {k}, field {q}"
            else:
                assert u.shape == v.shape and np.array_equal(u, v), f"{what}: scene {k}, field {q}"


def _twin_scenes():
    """Six scenes: step lengths 0.05 / 0.04 / 0.02 / 0.05 / 0.03 / 0.05, vehicle counts 0, 1, 4, 12, 4, 1 at full speed, one scene
    with its dynamic force off (its vehicles move all the same) and one without pedestrians."""
    counts = (0, 1, 4, 12, 4, 1)
    sizes = (30, 20, 64, 100, 0, 40)
    scenes = [_scene(n, 300 + k, m, slow=False) for k, (n, m) in enumerate(zip(sizes, counts))]
    cfgs = [_config(k, NO_DYN if k == 2 else ALL) for k in range(6)]
    dts = [0.05, 0.04, 0.02, 0.05, 0.03, 0.05]
    return scenes, cfgs, dts


def test_vehicles_track_the_host_twin():
    """Before each of 10 run(1), every scene's vehicles equal the twin advanced by that scene's dt bit for bit; the twin matches
    the oracle's float64 ring (O.ellipse_ring) to 4e-6."""
    scenes, cfgs, dts = _twin_scenes()
    b = _batch(scenes, cfgs, dts)
    try:
        moved = 0
        for t in range(10):
            for k, (sc, dev) in enumerate(zip(scenes, b.dynamic_obstacles())):
                _same_vehicles(dev, sc, f"scene {k} tick {t}")
                for j, (c, r) in enumerate(sc["dynamic_obstacles"]):
                    want = O.ellipse_ring(c, sc["dynamic_yaw"][j], *sc["dynamic_extent"][j])
                    assert np.max(np.abs(r - want)) <= 4e-6 * max(1.0, np.abs(want).max()), f"scene {k} tick {t}"
            start = [[c for c, _ in sc["dynamic_obstacles"]] for sc in scenes]
            b.run(1)
            for sc, dt in zip(scenes, dts):
                _advance(sc, dt)
            moved += sum(int(not np.array_equal(c0, c1)) for s0, sc in zip(start, scenes)
                         for c0, (c1, _) in zip(s0, sc["dynamic_obstacles"]))
        assert moved > 100, f"only {moved} vehicle moves in 10 ticks"
    finally:
        b.close()


@pytest.mark.parametrize("redraw", [False, True], ids=["plain", "redraw"])
@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_every_tick_matches_the_oracle(z_spread, redraw):
    """8 integrating ticks, every scene re-synchronised every tick against O.free_step with the twin's geometry: v' (plain 1e-5)
    and x' (1e-6)."""
    sizes, counts = (64, 30, 1, 0, 200), (4, 2, 1, 3, 12)
    scenes = [_scene(n, 700 + k, m, z_spread) for k, (n, m) in enumerate(zip(sizes, counts))]
    cfgs = [_config(k, ALL if k != 1 else NO_DYN) for k in range(5)]
    dts = [0.05, 0.04, 0.05, 0.02, 0.03]
    seeds, sides, thrs = [11, 12, 13, 14, 15], [0.3 * sc["world_side"] for sc in scenes], [3.0, 2.5, 2.0, 2.0, 4.0]
    b = _batch(scenes, cfgs, dts)
    try:
        assert b.planar == (z_spread == 0.0)
        if redraw:
            b.set_waypoint_streams(seeds, sides, thrs)
        for t in range(8):
            before = b.state()
            wps = b.waypoints()
            b.tick(integrate=True, redraw=redraw)
            after = b.state()
            for k, (sc, cfg, dt) in enumerate(zip(scenes, cfgs, dts)):
                n = len(sc["loc"])
                if n == 0:
                    continue
                loc, vel = before[k]
                wp3 = np.zeros((n, 3))
                wp3[:, :2] = wps[k][0]
                prm = O.OracleParams.from_config(cfg)
                geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"],
                                  dynamic_obstacles=sc["dynamic_obstacles"], dynamic_vel=sc["dynamic_vel"])
                crossing = np.zeros(n, bool)
                with np.errstate(all="ignore"):
                    oloc, ovel, _, _ = O.free_step(loc, vel, wp3, sc["target_speed"], sc["radius"], crossing,
                                                   wps[k][1].astype(np.int64), geom, prm, dt, arrive_threshold=thrs[k],
                                                   seed=seeds[k], world_side=sides[k], redraw=redraw, round_f32=True)
                    diag = {}
                    O.tick_forces(loc, vel, wp3, sc["target_speed"], sc["radius"], crossing, geom, prm,
                                  theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
                dloc, dvel = after[k]
                P.check_velocity(dvel, ovel, diag["total"][0], dt)
                assert np.max(np.abs(dloc - oloc)) <= 1e-6 * max(1.0, np.max(np.abs(oloc))) + 1e-6, f"scene {k} tick {t}"
            for sc, dt in zip(scenes, dts):
                _advance(sc, dt)
            for k, (sc, dev) in enumerate(zip(scenes, b.dynamic_obstacles())):
                _same_vehicles(dev, sc, f"scene {k} after tick {t}")
    finally:
        b.close()


def test_run_forms_agree():
    """run(K) == K x tick(integrate=True) bit for bit, pedestrians and vehicles; run_recorded frames == step-wise downloads of a
    second batch; a tick without SFM_TICK_INTEGRATE leaves every vehicle where it was."""
    scenes = [_scene(64, 41, 4), _scene(17, 42, 1), _scene(0, 43, 2), _scene(120, 44, 12)]
    cfgs = [_config(k, ALL) for k in range(4)]
    dts = [0.05, 0.04, 0.02, 0.05]
    A, B_, Cb, D = (_batch(scenes, cfgs, dts) for _ in range(4))
    try:
        A.run(7)
        for _ in range(7):
            B_.tick(integrate=True)
        _assert_same(_everything(A), _everything(B_), "run(7) vs 7 x tick")

        frames, idx, _ = Cb.run_recorded(9, stride=4)
        assert list(idx) == [0, 4, 8]
        want = [[] for _ in scenes]
        for k in (0, 4, 8):
            for s, (loc, vel) in enumerate(D.state()):
                want[s].append(np.float32(np.concatenate([loc[:, :2], vel[:, :2]], axis=1)))
            D.run(min(4, 9 - k))
        for s, sc in enumerate(scenes):
            assert np.array_equal(frames[s], np.stack(want[s]).reshape(3, len(sc["loc"]), 4)), f"scene {s}: frames"
        _assert_same(_everything(Cb), _everything(D), "run_recorded vs run")

        still = _everything(A)
        A.tick()
        A.tick()
        after = _everything(A)
        for k, (s0, s1) in enumerate(zip(still, after)):
            _assert_same([s0[2:]], [s1[2:]], f"non-integrating tick moved scene {k}'s vehicles")
        twin = [dict(sc) for sc in scenes]
        for sc, dt in zip(twin, dts):
            for _ in range(7):
                _advance(sc, dt)
        for k, (sc, dev) in enumerate(zip(twin, A.dynamic_obstacles())):
            _same_vehicles(dev, sc, f"scene {k} after 7 ticks and 2 non-integrating ticks")
    finally:
        for b in (A, B_, Cb, D):
            b.close()


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_scene_is_independent_of_the_batch(z_spread):
    """A scene with moving vehicles: pedestrians and vehicles bitwise the same alone and at position 3 of a batch of 7 mixed scenes
    (with and without vehicles, of other step lengths), over 12 ticks."""
    target = _scene(65, 77, 4, z_spread)
    tcfg, tdt = _config(3, ALL), 0.04
    others = [_scene(n, 1000 + k, m, z_spread) for k, (n, m) in enumerate(((30, 2), (0, 1), (130, 0), (1, 5), (64, 0), (250, 3)))]
    scenes = others[:3] + [target] + others[3:]
    cfgs = [_config(k, ALL) for k in range(3)] + [tcfg] + [_config(k, ALL) for k in range(3, 6)]
    dts = [0.05, 0.02, 0.05, tdt, 0.03, 0.05, 0.05]
    alone = _batch([target], [tcfg], [tdt], planar=z_spread == 0.0)
    mixed = _batch(scenes, cfgs, dts, planar=z_spread == 0.0)
    try:
        alone.run(5)
        mixed.run(5)
        alone.tick(integrate=True)
        mixed.tick(integrate=True)
        alone.run(6)
        mixed.run(6)
        _assert_same(_everything(alone), _everything(mixed)[3:4], "alone vs position 3")
        twin = dict(target)
        for _ in range(12):
            _advance(twin, tdt)
        _same_vehicles(alone.dynamic_obstacles()[0], twin, "target after 12 ticks")
    finally:
        alone.close()
        mixed.close()


def test_agrees_with_the_handle():
    """A one-scene batch and an SfmEngine with set_dynamic_boxes on the same scene: the vehicles bitwise equal after each of 10
    integrating ticks, v' within 1e-5 (the handle's sums are ordered differently; the handle is re-synchronised to the batch's
    state every tick)."""
    sc = _scene(64, 515, 4)
    cfg, dt = _config(0, ALL), 0.05
    b = _batch([sc], [cfg], [dt])
    eng = SfmEngine(cfg, dt)
    try:
        eng.set_borders(sc["borders"], sc["border_centers"], sc["border_lengths"])
        eng.set_static_obstacles(sc["static_obstacles"])
        eng.set_dynamic_boxes([c for c, _ in sc["dynamic_obstacles"]], sc["dynamic_yaw"], sc["dynamic_extent"], sc["dynamic_vel"])
        for t in range(10):
            (loc, vel), = b.state()
            wp = np.zeros((len(loc), 3))
            wp[:, :2] = b.waypoints()[0][0]
            eng.upload_state(loc, vel, wp, sc["target_speed"], sc["radius"], None)
            geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"],
                              dynamic_obstacles=b.dynamic_obstacles()[0], dynamic_vel=sc["dynamic_vel"])
            diag = {}
            with np.errstate(all="ignore"):
                O.tick_forces(loc, vel, wp, sc["target_speed"], sc["radius"], np.zeros(len(loc), bool), geom,
                              O.OracleParams.from_config(cfg), theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
            b.run(1)
            eng.run(1)
            hv = eng.state()[1]
            P.check_velocity(b.state()[0][1], hv, diag["total"][0], dt)
            hd, bd = eng.dynamic_obstacles(), b.dynamic_obstacles()[0]
            assert len(hd) == len(bd) == 4
            for j, ((c_h, r_h), (c_b, r_b)) in enumerate(zip(hd, bd)):
                assert np.array_equal(c_h, c_b) and np.array_equal(r_h, r_b), f"tick {t} vehicle {j}"
    finally:
        b.close()
        eng.close()


def test_switching_between_boxes_rings_and_nothing():
    """sfm_batch_set_dynamic_obstacles after boxes stops the motion; boxes without vehicles clear them (the batch then steps as
    one that never had any); upload() with the default device_vehicles=False replaces boxes with rings; sfm_batch_upload_state
    and set_params leave the vehicles where they are, and a new step length applies from the next integrating tick."""
    L = _lib.load()
    scenes = [_scene(40, 61, 3), _scene(25, 62, 0), _scene(50, 63, 5)]
    cfgs = [_config(k, ALL) for k in range(3)]
    dts = [0.05, 0.04, 0.02]
    b = _batch(scenes, cfgs, dts)
    try:
        b.run(3)
        for sc, dt in zip(scenes, dts):
            for _ in range(3):
                _advance(sc, dt)
        # sfm_batch_upload_state through the C ABI, then set_params with other step lengths: the vehicles stay
        pk = pack_scenes(scenes)
        f = lambda key: pk[key].ctypes.data
        assert L.sfm_batch_upload_state(b._b, pk["scene_off"].ctypes.data, f("x"), f("y"), None, f("vx"), f("vy"), None, f("wx"),
                                        f("wy"), f("target_speed"), f("radius"), pk["crossing"].ctypes.data) == 0
        for k, (sc, dev) in enumerate(zip(scenes, b.dynamic_obstacles())):
            _same_vehicles(dev, sc, f"scene {k} after sfm_batch_upload_state")
        new_dts = [0.03, 0.05, 0.045]
        b.set_params(cfgs, new_dts)
        for k, (sc, dev) in enumerate(zip(scenes, b.dynamic_obstacles())):
            _same_vehicles(dev, sc, f"scene {k} after set_params")
        b.run(2)
        for sc, dt in zip(scenes, new_dts):
            _advance(sc, dt)
            _advance(sc, dt)
        for k, (sc, dev) in enumerate(zip(scenes, b.dynamic_obstacles())):
            _same_vehicles(dev, sc, f"scene {k} advanced by the new step length")

        # rings through sfm_batch_set_dynamic_obstacles: from then on the vehicles stay where they were set
        dy = pack_scenes(scenes)["dynamic"]
        assert L.sfm_batch_set_dynamic_obstacles(b._b, *(a.ctypes.data for a in dy)) == 0
        b.run(3)
        for k, (sc, dev) in enumerate(zip(scenes, b.dynamic_obstacles())):
            _same_vehicles(dev, sc, f"scene {k}: rings do not move")

        # boxes again, then boxes without vehicles: every vehicle is gone and the batch steps as one without any
        b.set_dynamic_boxes(scenes)
        bare = [dict(sc, dynamic_obstacles=[], dynamic_vel=None, dynamic_yaw=None, dynamic_extent=None) for sc in scenes]
        b.set_dynamic_boxes(bare)
        assert b.dynamic_obstacles() == [[], [], []]
        b.upload_packed(pack_scenes(scenes))        # (vehicles as rings again, pedestrians back to the start)
        b.set_dynamic_boxes(bare)
        ref = SfmBatch(cfgs, new_dts)
        try:
            ref.upload(bare)
            b.run(4)
            ref.run(4)
            _assert_same(b.state(), ref.state(), "boxes without vehicles vs a batch without vehicles")
        finally:
            ref.close()

        # boxes replaced by upload()'s rings: the scenes' rings as given, and they stay
        b.set_dynamic_boxes(scenes)
        b.run(2)
        b.upload(scenes)
        given = [[(np.float32(c).astype(np.float64), np.float32(r).astype(np.float64)) for c, r in sc["dynamic_obstacles"]]
                 for sc in scenes]
        b.run(2)
        for k, (g, dev) in enumerate(zip(given, b.dynamic_obstacles())):
            _same_vehicles(dev, {"dynamic_obstacles": g}, f"scene {k}: upload() rings")
    finally:
        b.close()


def test_refusals_leave_the_batch_usable():
    """Each bad input of sfm_batch_set_dynamic_boxes returns SFM_ERR_INVALID with a message and changes nothing; afterwards the
    batch ticks exactly as a fresh batch does."""
    L = _lib.load()
    scenes = [_scene(20, 81, 2), _scene(10, 82, 3)]
    cfgs = [_config(0, ALL), _config(1, ALL)]
    dts = [0.05, 0.04]
    b = _batch(scenes, cfgs, dts)
    fresh = _batch(scenes, cfgs, dts)
    try:
        h = b._b
        before = _everything(b)
        good = list(pack_boxes(scenes))
        p = lambda a: None if a is None else a.ctypes.data

        def call(args):
            return L.sfm_batch_set_dynamic_boxes(h, *(p(a) for a in args))

        def bad(i, a):
            args = list(good)
            args[i] = a
            return args

        io, off = good[0], good[1]
        cases = [
            (bad(0, None), "NULL"),
            (bad(0, np.array([1, 2, 5], np.int32)), "[0] must be 0"),
            (bad(0, np.array([0, 3, 2], np.int32)), "non-decreasing"),
            (bad(1, None), "NULL"),
            (bad(1, (off + 1).astype(np.int32)), "[0] must be 0"),
            (bad(1, np.concatenate([off[:2], off[1:2] - 1, off[3:]]).astype(np.int32)), "non-decreasing"),
            (bad(2, None), "NULL"), (bad(3, None), "NULL"),
            (bad(4, None), "NULL"), (bad(5, None), "NULL"),
            (bad(6, None), "NULL"), (bad(7, None), "NULL"),
            (bad(8, None), "together"), (bad(9, None), "together"),
        ]
        assert io.tolist() == [0, 2, 5]
        for k, (args, msg) in enumerate(cases):
            assert call(args) == -1, f"case {k}"            # SFM_ERR_INVALID
            err = L.sfm_batch_last_error(h).decode()
            assert msg in err, f"case {k}: {err!r}"
        _assert_same(_everything(b), before, "after the refused calls")
        b.run(5)
        fresh.run(5)
        _assert_same(_everything(b), _everything(fresh), "refused calls vs a fresh batch")
    finally:
        b.close()
        fresh.close()


def test_at_size():
    """256 scenes x 64 pedestrians x 4 vehicles, all five forces, 20 ticks: every vehicle equals the twin bit for bit; 8 scenes
    match the oracle on the last tick."""
    B = 256
    scenes = [_scene(64, 5000 + k, 4, borders=2, static=1) for k in range(B)]
    cfgs = [_config(k % 4, ALL) for k in range(B)]
    dts = [(0.05, 0.04, 0.02, 0.03)[k % 4] for k in range(B)]
    b = _batch(scenes, cfgs, dts)
    try:
        b.run(19)
        for sc, dt in zip(scenes, dts):
            for _ in range(19):
                _advance(sc, dt)
        before = b.state()
        wps = b.waypoints()
        b.run(1)
        after = b.state()
        sample = [0, 37, 64, 101, 128, 190, 222, 255]
        for k in sample:
            sc, cfg, dt = scenes[k], cfgs[k], dts[k]
            loc, vel = before[k]
            wp3 = np.zeros((64, 3))
            wp3[:, :2] = wps[k][0]
            prm = O.OracleParams.from_config(cfg)
            geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"],
                              dynamic_obstacles=sc["dynamic_obstacles"], dynamic_vel=sc["dynamic_vel"])
            diag = {}
            with np.errstate(all="ignore"):
                oloc, ovel, _, _ = O.free_step(loc, vel, wp3, sc["target_speed"], sc["radius"], np.zeros(64, bool),
                                               np.zeros(64, np.int64), geom, prm, dt, redraw=False, round_f32=True)
                O.tick_forces(loc, vel, wp3, sc["target_speed"], sc["radius"], np.zeros(64, bool), geom, prm,
                              theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
            P.check_velocity(after[k][1], ovel, diag["total"][0], dt)
            assert np.max(np.abs(after[k][0] - oloc)) <= 1e-6 * max(1.0, np.max(np.abs(oloc))) + 1e-6, f"scene {k}"
        for sc, dt in zip(scenes, dts):
            _advance(sc, dt)
        for k, (sc, dev) in enumerate(zip(scenes, b.dynamic_obstacles())):
            _same_vehicles(dev, sc, f"scene {k} after 20 ticks")
    finally:
        b.close()
