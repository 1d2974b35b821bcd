"""GPU tests of batched scenes (sfm_batch_* through carla_social_force_model_amd.batch): per-scene parity with the oracle, bitwise
batch invariance, agreement with the single-crowd handle, multi-tick runs, and input errors.
Run on the MI355X box with  python -m pytest tests -m gpu."""
import ctypes as C

import numpy as np
import pytest

import _parity as P
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import SfmBatch, batch_params, pack_scenes
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.engine import SfmEngine
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

GEO = ("acceleration_force", "pedestrian_force", "border_force", "static_obstacle_force")


def _scene(n, seed, z_spread=0.0, geo=True, dynamic=0, crossing=False):
    sc = vars(scenarios.make_scenario(n, seed, n_borders=6 if geo else 0, n_static=3 if geo else 0, n_dynamic=dynamic,
                                      z_spread=z_spread, border_len=(3.0, 15.0)))
    rng = np.random.default_rng(seed + 17)
    sc["radius"] = np.float32(rng.uniform(0.2, 0.45, n)).astype(np.float64)
    if crossing:
        sc["crossing"] = rng.random(n) < 0.2
    return sc


def _config(k, forces):
    cfg = default_sfm_config(forces)
    cfg["pedestrian_force"].update({"A": 3.0 + 0.5 * k, "lambda": 1.5 + 0.1 * k, "gamma": 0.3 + 0.02 * k})
    cfg["goal_force"] = {"tau": 0.4 + 0.05 * k}
    cfg["use_ped_radius"] = bool(k % 2)
    return cfg


def _oracle(sc, cfg, dt):
    """(v' reference, exposure, summed term magnitudes) of one scene."""
    n = len(sc["loc"])
    prm = O.OracleParams.from_config(cfg)
    geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"], sc["dynamic_obstacles"],
                      sc["dynamic_vel"])
    crossing = sc.get("crossing")
    crossing = np.zeros(n, bool) if crossing is None else crossing
    diag = {}
    with np.errstate(all="ignore"):
        _, total, _ = O.tick_forces(sc["loc"], sc["vel"], sc["waypoint"], sc["target_speed"], sc["radius"], crossing, geom, prm,
                                    theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
    v = O.new_velocities(sc["vel"], total, sc["target_speed"], dt, prm.max_speed_factor)
    summed = sum(np.nan_to_num(ab) for name, (_, ab) in diag.items() if name != "total")
    return v, diag["total"][0], summed


def _run_batch(scenes, cfgs, dts, ticks=0, integrate=False):
    b = SfmBatch(cfgs, dts)
    try:
        b.upload(scenes)
        if ticks:
            b.run(ticks)
        else:
            b.tick(integrate=integrate)
        return b.state(), b.planar
    finally:
        b.close()


SIZES = [0, 1, 2, 3, 17, 64, 65, 256, 1000, 1024]


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_every_scene_matches_the_oracle(z_spread):
    """One batch of mixed sizes, every scene with its own parameters (A, lambda, gamma, tau, dt, use_ped_radius, which forces), a
    coincident pair, a crossing mask: v' of every scene against the oracle (plain 1e-5), plus two scenes with vehicles (the
    conditioned bound of the handle's dynamic-obstacle tests)."""
    force_sets = [GEO, ("acceleration_force", "pedestrian_force"), ("pedestrian_force", "border_force", "static_obstacle_force"),
                  ("acceleration_force", "border_force")]
    scenes, cfgs, dts = [], [], []
    for k, n in enumerate(SIZES):
        forces = force_sets[k % len(force_sets)]
        sc = _scene(n, 300 + k, z_spread, geo="border_force" in forces, crossing=k % 3 == 0)
        if n == 17:
            sc["loc"][5] = sc["loc"][6]                       # a coincident pair (different velocities)
        scenes.append(sc)
        cfgs.append(_config(k, forces))
        dts.append([0.05, 0.04, 0.02][k % 3])
    dyn_first = len(scenes)
    for k, n in enumerate((40, 300)):
        scenes.append(_scene(n, 400 + k, z_spread, dynamic=3))
        cfgs.append(_config(k, scenarios.ALL_FORCES))
        dts.append(0.05)
    (states, planar) = _run_batch(scenes, cfgs, dts)
    assert planar == (z_spread == 0.0)
    for k, (sc, cfg, dt) in enumerate(zip(scenes, cfgs, dts)):
        loc, vel = states[k]
        assert loc.shape == (len(sc["loc"]), 3)
        if len(sc["loc"]) == 0:
            continue
        np.testing.assert_array_equal(loc, np.float32(sc["loc"]))       # no integration: x unchanged (z too)
        v_ref, expo, summed = _oracle(sc, cfg, dt)
        if k >= dyn_first:
            needed = P.check_velocity_conditioned(vel, v_ref, expo, summed, dt)
            assert needed <= max(2, len(sc["loc"]) // 100), f"scene {k}"
        else:
            P.check_velocity(vel, v_ref, expo, dt)


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_scene_result_is_independent_of_the_rest_of_the_batch(z_spread):
    """Scene k's v' bit for bit: alone (B = 1), first in a batch of 1000 other scenes, and at position 700 of it."""
    target = _scene(65, 77, z_spread, crossing=True)
    tcfg = _config(3, GEO)
    rng = np.random.default_rng(5)
    others = [_scene(int(rng.integers(0, 130)), 1000 + k, z_spread, geo=k % 4 == 0) for k in range(1000)]
    ocfg = [_config(k % 7, GEO if k % 4 == 0 else ("acceleration_force", "pedestrian_force")) for k in range(1000)]
    alone, _ = _run_batch([target], [tcfg], [0.04])
    first, _ = _run_batch([target] + others, [tcfg] + ocfg, [0.04] + [0.05] * 1000)
    mid, _ = _run_batch(others[:700] + [target] + others[700:], ocfg[:700] + [tcfg] + ocfg[700:], [0.05] * 700 + [0.04] + [0.05] * 300)
    assert np.array_equal(alone[0][1], first[0][1])
    assert np.array_equal(alone[0][1], mid[700][1])
    assert np.array_equal(alone[0][0], mid[700][0])


def test_batch_agrees_with_the_handle():
    """Each scene stepped through its own SfmEngine handle agrees with the batch to 1e-5 (the sums are ordered differently)."""
    sizes = [1, 17, 64, 200, 1000]
    scenes = [_scene(n, 500 + k, crossing=True) for k, n in enumerate(sizes)]
    cfgs = [_config(k, GEO) for k in range(len(sizes))]
    dts = [0.05, 0.03, 0.05, 0.04, 0.05]
    states, _ = _run_batch(scenes, cfgs, dts)
    for k, (sc, cfg, dt) in enumerate(zip(scenes, cfgs, dts)):
        eng = SfmEngine(cfg, dt)
        try:
            eng.set_borders(sc["borders"], sc["border_centers"], sc["border_lengths"])
            eng.set_static_obstacles(sc["static_obstacles"])
            eng.upload_state(sc["loc"], sc["vel"], sc["waypoint"], sc["target_speed"], sc["radius"], sc["crossing"])
            eng.tick()
            v_handle = eng.velocities()
        finally:
            eng.close()
        _, expo, _ = _oracle(sc, cfg, dt)
        P.check_velocity(states[k][1], v_handle, expo, dt)


def test_multi_tick_runs():
    """40 integrating ticks re-synchronised every tick against O.free_step (1e-5); run(40) equals 40 x tick(integrate=True) bit
    for bit; two identical runs are identical."""
    scenes = [_scene(50, 601), _scene(200, 602, crossing=True), _scene(0, 603), _scene(7, 604, geo=False)]
    cfgs = [_config(k, GEO if k != 3 else ("acceleration_force", "pedestrian_force")) for k in range(4)]
    dts = [0.05, 0.04, 0.05, 0.02]
    b = SfmBatch(cfgs, dts)
    try:
        b.upload(scenes)
        cur = [(np.float32(sc["loc"]).astype(np.float64), np.float32(sc["vel"]).astype(np.float64)) for sc in scenes]
        for t in range(40):
            b.tick(integrate=True)
            got = b.state()
            for k, (sc, cfg, dt) in enumerate(zip(scenes, cfgs, dts)):
                n = len(sc["loc"])
                if n == 0:
                    continue
                loc, vel = cur[k]
                prm = O.OracleParams.from_config(cfg)
                geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"], [], None)
                crossing = sc.get("crossing")
                crossing = np.zeros(n, bool) if crossing is None else crossing
                with np.errstate(all="ignore"):
                    oloc, ovel, _, _ = O.free_step(loc, vel, sc["waypoint"], sc["target_speed"], sc["radius"], crossing,
                                                   np.zeros(n, np.int64), geom, prm, dt, redraw=False, round_f32=True)
                    diag = {}
                    O.tick_forces(loc, vel, sc["waypoint"], sc["target_speed"], sc["radius"], crossing, geom, prm,
                                  theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
                dloc, dvel = got[k]
                P.check_velocity(dvel, ovel, diag["total"][0], dt)
                assert np.max(np.abs(dloc - oloc)) <= 1e-6 * max(1.0, np.max(np.abs(oloc))) + 1e-6, f"scene {k} tick {t}"
                cur[k] = (dloc, dvel)                          # continue from the device's fp32 state
        stepped = b.state()
    finally:
        b.close()
    ran, _ = _run_batch(scenes, cfgs, dts, ticks=40)
    again, _ = _run_batch(scenes, cfgs, dts, ticks=40)
    for k in range(len(scenes)):
        for q in range(2):
            assert np.array_equal(ran[k][q], stepped[k][q]), f"scene {k}: run(40) != 40 ticks"
            assert np.array_equal(ran[k][q], again[k][q]), f"scene {k}: two runs differ"


def test_bad_input_is_refused_and_the_batch_stays_usable():
    L = _lib.load()
    prm = batch_params(default_sfm_config(("acceleration_force", "pedestrian_force")), 0.05, B=2)
    h = C.c_void_p()
    assert L.sfm_batch_create(0, prm, 0, C.byref(h)) != 0 and b"B must be" in L.sfm_batch_last_error(None)
    assert L.sfm_batch_create(2, prm, 0, C.byref(h)) == 0
    try:
        sc = [_scene(5, 1, geo=False), _scene(3, 2, geo=False)]
        pk = pack_scenes(sc)
        f = lambda k: pk[k].ctypes.data

        def upload(scene_off, x=None):
            so = np.ascontiguousarray(scene_off, dtype=np.int32)
            return L.sfm_batch_upload_state(h, so.ctypes.data, f("x") if x is None else x, f("y"), None, f("vx"), f("vy"), None,
                                            f("wx"), f("wy"), f("target_speed"), None, None)

        def err():
            return L.sfm_batch_last_error(h).decode()

        assert L.sfm_batch_tick(h, 0) != 0 and "upload" in err()            # no state yet
        assert upload([0, 5, 3]) != 0 and "non-decreasing" in err()
        assert upload([1, 5, 8]) != 0 and "[0] must be 0" in err()
        big = np.zeros(1025, np.float32)
        assert upload([0, 1025, 1025], x=big.ctypes.data) != 0 and "1024" in err()
        so = np.array([0, 5, 8], np.int32)
        assert L.sfm_batch_upload_state(h, so.ctypes.data, None, f("y"), None, f("vx"), f("vy"), None, f("wx"), f("wy"),
                                        f("target_speed"), None, None) != 0 and "NULL" in err()
        assert L.sfm_batch_upload_state(h, None, f("x"), f("y"), None, f("vx"), f("vy"), None, f("wx"), f("wy"),
                                        f("target_speed"), None, None) != 0 and "NULL" in err()
        item = np.array([0, 1, 3], np.int32)
        off = np.array([0, 4, 2, 6], np.int32)                 # polyline offsets going backwards
        pts = np.zeros(6, np.float32)
        assert L.sfm_batch_set_static_obstacles(h, item.ctypes.data, off.ctypes.data, pts.ctypes.data, pts.ctypes.data,
                                                pts.ctypes.data, pts.ctypes.data) != 0 and "offsets" in err()
        assert upload([0, 5, 8]) == 0
        assert L.sfm_batch_tick(h, _lib.TICK_REDRAW_WAYPOINTS) != 0 and "SFM_TICK_INTEGRATE" in err()
        assert L.sfm_batch_run(h, 3, _lib.TICK_INTEGRATE | _lib.TICK_RECORD_FORCES) != 0 and "SFM_TICK_INTEGRATE" in err()
        assert L.sfm_batch_run(h, -1, 0) != 0
        # the next valid calls still work
        assert L.sfm_batch_tick(h, 0) == 0
        vx = np.full(8, np.nan, np.float32)
        assert L.sfm_batch_download_state(h, None, None, None, vx.ctypes.data, None, None) == 0
        assert np.isfinite(vx).all()
    finally:
        L.sfm_batch_destroy(h)
    # ... and through the Python layer: SfmLibraryError, never a CPU fallback
    b = SfmBatch(default_sfm_config(("acceleration_force", "pedestrian_force")), 0.05, B=1)
    try:
        with pytest.raises(_lib.SfmLibraryError):
            b.tick()                                           # nothing uploaded
        pk = pack_scenes([_scene(3, 1, geo=False)])
        pk["scene_off"] = np.array([0, 1025], np.int32)        # bypass pack_scenes' own check
        with pytest.raises(_lib.SfmLibraryError, match="1024"):
            b.upload_packed(pk)
        b.upload([_scene(3, 1, geo=False)])
        b.tick(integrate=True)
        assert np.isfinite(b.state()[0][1]).all()
    finally:
        b.close()
