"""CPU-side checks of the batched-scenes layer (carla_social_force_model_amd.batch): packing of many scenes into the concatenated
SoA / CSR arrays of the C ABI, the planar decision, input validation, per-scene parameters.  No GPU needed."""
import numpy as np
import pytest

from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd.batch import MAX_SCENE_PEDESTRIANS, batch_params, pack_scenes
from carla_social_force_model_amd.config import default_sfm_config


def _scene(n, seed, **kw):
    return vars(scenarios.make_scenario(n, seed, **kw))


def test_offsets_and_concatenation_for_mixed_sizes():
    sizes = [3, 0, 1, 17, 0, 64]
    scenes = [_scene(n, 10 + k) for k, n in enumerate(sizes)]
    scenes[2]["crossing"] = np.array([True])
    pk = pack_scenes(scenes)
    assert pk["scene_off"].dtype == np.int32
    assert pk["scene_off"].tolist() == [0, 3, 3, 4, 21, 21, 85]
    for key in ("x", "y", "z", "vx", "vy", "vz", "wx", "wy", "target_speed", "radius"):
        assert pk[key].dtype == np.float32 and pk[key].shape == (85,), key
    assert pk["crossing"].dtype == np.uint8 and pk["crossing"].tolist() == [0, 0, 0, 1] + [0] * 81
    for b, sc in enumerate(scenes):
        lo, hi = pk["scene_off"][b], pk["scene_off"][b + 1]
        np.testing.assert_array_equal(pk["x"][lo:hi], np.float32(sc["loc"][:, 0]))
        np.testing.assert_array_equal(pk["y"][lo:hi], np.float32(sc["loc"][:, 1]))
        np.testing.assert_array_equal(pk["vy"][lo:hi], np.float32(sc["vel"][:, 1]))
        np.testing.assert_array_equal(pk["wx"][lo:hi], np.float32(sc["waypoint"][:, 0]))
        np.testing.assert_array_equal(pk["target_speed"][lo:hi], np.float32(sc["target_speed"]))
        np.testing.assert_array_equal(pk["radius"][lo:hi], np.float32(sc["radius"]))


def test_missing_radius_and_crossing_default_to_zero():
    sc = _scene(5, 1)
    sc["radius"] = None
    pk = pack_scenes([{k: sc[k] for k in ("loc", "vel", "waypoint", "target_speed", "radius")}])
    assert pk["radius"].tolist() == [0.0] * 5 and pk["crossing"].tolist() == [0] * 5
    assert pk["borders"][0].tolist() == [0, 0] and pk["static"][0].tolist() == [0, 0] and pk["dynamic"][0].tolist() == [0, 0]


def test_geometry_csr_per_scene():
    a = _scene(4, 1, n_borders=3, n_static=2, n_dynamic=1)
    b = _scene(2, 2)                                     # no geometry at all
    c = _scene(6, 3, n_borders=1, n_dynamic=2)
    pk = pack_scenes([a, b, c])
    item, off, px, py, cx, cy, ln = pk["borders"]
    assert item.tolist() == [0, 3, 3, 4]
    polys = a["borders"] + c["borders"]
    assert off.tolist() == [0] + np.cumsum([len(p) for p in polys]).tolist()
    np.testing.assert_array_equal(px, np.float32(np.concatenate(polys)[:, 0]))
    np.testing.assert_array_equal(py, np.float32(np.concatenate(polys)[:, 1]))
    np.testing.assert_array_equal(cx, np.float32(np.concatenate([a["border_centers"], c["border_centers"]])[:, 0]))
    np.testing.assert_array_equal(ln, np.float32(np.concatenate([a["border_lengths"], c["border_lengths"]])))
    item, off, px, py, cx, cy = pk["static"]
    assert item.tolist() == [0, 2, 2, 2]
    assert off.tolist() == [0, len(a["static_obstacles"][0][1]), len(a["static_obstacles"][0][1]) + len(a["static_obstacles"][1][1])]
    np.testing.assert_array_equal(cy, np.float32([o[0][1] for o in a["static_obstacles"]]))
    item, off, px, py, cx, cy, vx, vy = pk["dynamic"]
    assert item.tolist() == [0, 1, 1, 3]
    assert len(off) == 4 and off[-1] == len(px) == sum(len(o[1]) for o in a["dynamic_obstacles"] + c["dynamic_obstacles"])
    np.testing.assert_array_equal(vx, np.float32(np.concatenate([a["dynamic_vel"], c["dynamic_vel"]])[:, 0]))
    for arr in pk["borders"][:2] + pk["static"][:2] + pk["dynamic"][:2]:
        assert arr.dtype == np.int32


def test_dynamic_obstacles_without_velocities_are_at_rest():
    sc = _scene(3, 5, n_dynamic=2)
    sc["dynamic_vel"] = None
    vx, vy = pack_scenes([sc])["dynamic"][6:]
    assert vx.tolist() == [0.0, 0.0] and vy.tolist() == [0.0, 0.0]


def test_planar_decision():
    flat = _scene(10, 1)
    lifted = _scene(10, 2)
    lifted["loc"] = lifted["loc"].copy()
    lifted["loc"][:, 2] = 1.5                         # a common z other than 0: still planar
    assert pack_scenes([flat, lifted])["planar"]
    spread = _scene(10, 3, z_spread=1.0)              # z differs inside one scene
    assert not pack_scenes([flat, spread])["planar"]
    climbing = _scene(10, 4)
    climbing["vel"] = climbing["vel"].copy()
    climbing["vel"][3, 2] = 0.1                       # one v_z
    assert not pack_scenes([climbing, flat])["planar"]
    assert pack_scenes([_scene(0, 1), _scene(1, 2)])["planar"]


def test_scene_size_limit_and_malformed_input():
    assert MAX_SCENE_PEDESTRIANS == 1024
    pack_scenes([_scene(1024, 1)])
    with pytest.raises(ValueError, match="1025 pedestrians"):
        pack_scenes([_scene(3, 1), _scene(1025, 2)])
    with pytest.raises(ValueError):
        pack_scenes([])
    bad = _scene(4, 1, n_borders=3)
    bad["border_lengths"] = bad["border_lengths"][:2]
    with pytest.raises(ValueError, match="borders need"):
        pack_scenes([bad])
    bad = _scene(4, 1, n_borders=2)
    bad["border_centers"] = bad["border_centers"][:1]
    with pytest.raises(ValueError, match="borders need"):
        pack_scenes([bad])
    bad = _scene(4, 1, n_borders=1)
    bad["borders"] = [np.zeros((5, 3))]
    with pytest.raises(ValueError, match=r"\(P,2\)"):
        pack_scenes([bad])
    bad = _scene(4, 1, n_dynamic=2)
    bad["dynamic_vel"] = bad["dynamic_vel"][:1]
    with pytest.raises(ValueError, match="velocities"):
        pack_scenes([bad])
    bad = _scene(4, 1, n_static=1)
    bad["static_obstacles"] = [(np.zeros(2),)]
    with pytest.raises(ValueError, match="center, ring"):
        pack_scenes([bad])
    bad = _scene(4, 1)
    bad["vel"] = bad["vel"][:3]
    with pytest.raises(ValueError, match="vel"):
        pack_scenes([bad])


def test_per_scene_params_from_different_configs():
    cfgs = []
    for k in range(4):
        cfg = default_sfm_config(("acceleration_force", "pedestrian_force") + (("border_force",) if k % 2 else ()))
        cfg["pedestrian_force"]["A"] = 2.0 + k
        cfg["pedestrian_force"]["lambda"] = 1.0 + 0.5 * k
        cfg["goal_force"] = {"tau": 0.3 + 0.1 * k}
        cfg["use_ped_radius"] = k == 3
        cfgs.append(cfg)
    prm = batch_params(cfgs, [0.05, 0.04, 0.03, 0.02])
    assert len(prm) == 4
    for k, p in enumerate(prm):
        assert p.pedestrian.A == pytest.approx(2.0 + k)
        assert p.pedestrian.lambda_ == pytest.approx(1.0 + 0.5 * k)
        assert p.tau == pytest.approx(0.3 + 0.1 * k)
        assert p.step_length == pytest.approx([0.05, 0.04, 0.03, 0.02][k])
        assert p.use_ped_radius == int(k == 3)
        assert list(p.enabled) == [1, 1, k % 2, 0, 0]
    one = batch_params(default_sfm_config(), 0.05, B=3)           # one config for every scene
    assert len(one) == 3 and all(p.step_length == pytest.approx(0.05) for p in one)
    with pytest.raises(ValueError):
        batch_params(cfgs, [0.05, 0.04])
