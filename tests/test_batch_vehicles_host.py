"""CPU-side checks of the batch's device-side vehicles (carla_social_force_model_amd.batch.pack_boxes): per scene, the arguments of
sfm_batch_set_dynamic_boxes are exactly what SfmEngine.set_dynamic_boxes passes to sfm_set_dynamic_boxes for that scene alone
(CSR, ring-local offsets, the bits of cos / sin), empty scenes and scenes without vehicles, refused input, and the ABI 8
declarations.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import pack_boxes
from carla_social_force_model_amd.engine import SfmEngine


class _Recorder:
    """Stands in for the library: copies out the arrays SfmEngine.set_dynamic_boxes passes to sfm_set_dynamic_boxes, during the
    call (they are temporaries of the caller)."""

    def __init__(self):
        self.args = None

    def sfm_set_dynamic_boxes(self, h, M, off, ux, uy, cx, cy, yc, ys, vx, vy):
        if M == 0:
            self.args = None
            return 0
        arr = lambda p, n, t: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(n,)).copy() if n else np.zeros(0, np.float32)
        o = arr(off, M + 1, C.c_int32)
        P = int(o[-1])
        self.args = (o, *(arr(p, n, C.c_float) for p, n in zip((ux, uy, cx, cy, yc, ys, vx, vy), (P, P, M, M, M, M, M, M))))
        return 0


def _handle_args(sc):
    """(offsets, ux, uy, cx, cy, cos, sin, vx, vy) SfmEngine.set_dynamic_boxes passes for the scene alone (None: no vehicles)."""
    eng = SfmEngine.__new__(SfmEngine)
    rec = _Recorder()
    eng._lib, eng._h = rec, None
    eng._check = lambda rc, what: None
    eng.set_dynamic_boxes([c for c, _ in sc["dynamic_obstacles"]], sc["dynamic_yaw"], sc["dynamic_extent"], sc["dynamic_vel"])
    return rec.args


def _scene(n, seed, dynamic):
    return vars(scenarios.make_scenario(n, seed, n_dynamic=dynamic))


def test_every_scene_packs_what_the_handle_passes():
    scenes = [_scene(10, 1, 4), _scene(0, 2, 0), _scene(5, 3, 0), _scene(0, 4, 3), _scene(20, 5, 12), _scene(3, 6, 1)]
    scenes[4]["dynamic_extent"] = np.tile([[2.4, 1.0], [0.6, 0.3], [4.0, 1.8]], (4, 1))   # rings of different lengths
    item_off, off, ux, uy, cx, cy, yc, ys, vx, vy = pack_boxes(scenes)
    assert item_off.dtype == np.int32 and off.dtype == np.int32
    assert item_off.tolist() == [0, 4, 4, 4, 7, 19, 20]
    for a in (ux, uy, cx, cy, yc, ys, vx, vy):
        assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    assert len(off) == 21 and len(ux) == len(uy) == off[-1] and len(cx) == 20
    for b, sc in enumerate(scenes):
        k0, k1 = item_off[b], item_off[b + 1]
        want = _handle_args(sc)
        if want is None:
            assert k0 == k1
            continue
        woff, wux, wuy, wcx, wcy, wyc, wys, wvx, wvy = want
        p0 = off[k0]
        assert np.array_equal(off[k0:k1 + 1] - p0, woff), f"scene {b}: offsets"
        for name, got, exp in (("ux", ux[p0:off[k1]], wux), ("uy", uy[p0:off[k1]], wuy), ("cx", cx[k0:k1], wcx),
                               ("cy", cy[k0:k1], wcy), ("cos", yc[k0:k1], wyc), ("sin", ys[k0:k1], wys),
                               ("vx", vx[k0:k1], wvx), ("vy", vy[k0:k1], wvy)):
            assert got.view(np.uint32).tolist() == exp.view(np.uint32).tolist(), f"scene {b}: {name}"
        # the fp32 cos / sin of the float64 yaw, the host twin's rotation (scenarios.place_ring_f32)
        assert np.array_equal(yc[k0:k1], np.float32(np.cos(sc["dynamic_yaw"])))


def test_scenes_without_vehicles():
    item_off, off, ux, uy, *rest = pack_boxes([_scene(4, 1, 0), {"loc": np.zeros((0, 3))}, _scene(0, 2, 0)])
    assert item_off.tolist() == [0, 0, 0, 0] and off.tolist() == [0]
    assert all(a.size == 0 for a in (ux, uy, *rest))
    item_off, off, *_ = pack_boxes([])
    assert item_off.tolist() == [0] and off.tolist() == [0]


def test_velocity_defaults_to_rest():
    sc = _scene(2, 3, 2)
    sc["dynamic_vel"] = None
    *_, vx, vy = pack_boxes([sc])
    assert vx.tolist() == [0.0, 0.0] and vy.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("key,value", [("dynamic_yaw", np.zeros(3)), ("dynamic_extent", np.ones((5, 2))),
                                       ("dynamic_vel", np.zeros((2, 2))), ("dynamic_yaw", None), ("dynamic_extent", None)])
def test_count_mismatches_raise(key, value):
    sc = _scene(2, 7, 4)
    sc[key] = value
    with pytest.raises(ValueError, match=f"scene 1.*{key}"):
        pack_boxes([_scene(1, 8, 1), sc])


def test_malformed_vehicle_raises():
    sc = _scene(2, 7, 2)
    sc["dynamic_obstacles"] = [sc["dynamic_obstacles"][0], (np.zeros(2),)]
    with pytest.raises(ValueError, match="scene 0"):
        pack_boxes([sc])


def test_abi8_entry_points_are_declared():
    assert _lib.ABI_VERSION >= 8
    for name in ("sfm_batch_set_dynamic_boxes", "sfm_batch_download_dynamic_obstacles"):
        assert name in _lib.SYMBOLS and _lib.SINCE[name] == 8
    assert len(_lib.SYMBOLS["sfm_batch_set_dynamic_boxes"][1]) == 11
    assert len(_lib.SYMBOLS["sfm_batch_download_dynamic_obstacles"][1]) == 5
