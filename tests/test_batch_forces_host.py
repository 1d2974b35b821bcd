"""CPU tests of the batch force-record helpers (batch.force_mask, split_forces, record_bytes) and the ABI that carries them."""
import numpy as np
import pytest

from carla_social_force_model_amd import _lib
from carla_social_force_model_amd.batch import (FORCE_RECORD_NAMES, MAX_RECORD_BYTES, force_mask, n_frames, record_bytes,
                                                split_forces)


def test_names_are_the_reference_dict_keys_and_the_total():
    assert FORCE_RECORD_NAMES == ("acceleration_force", "pedestrian_force", "border_force", "static_obstacle_force",
                                  "dynamic_obstacle_force", "total")
    assert FORCE_RECORD_NAMES.index("total") == _lib.FORCE_TOTAL


def test_force_mask_bits():
    assert force_mask() == 0x3F
    assert force_mask("total") == 1 << 5
    assert force_mask(["dynamic_obstacle_force", "acceleration_force"]) == 0b10001
    assert force_mask(("border_force", "border_force")) == 0b100
    for k, name in enumerate(FORCE_RECORD_NAMES):
        assert force_mask([name]) == 1 << k
    for bad in ([], ("goal_force",), ["total", "nope"]):
        with pytest.raises(ValueError):
            force_mask(bad)


def test_split_forces_shapes_and_order():
    so = np.array([0, 3, 3, 7], np.int32)
    names = ("total", "pedestrian_force")                       # given out of order: the record is in index order
    buf = np.arange(2 * 7 * 2, dtype=np.float32).reshape(2, 7, 2)
    out = split_forces(buf, so, names)
    assert len(out) == 3
    for b, d in enumerate(out):
        assert list(d) == ["pedestrian_force", "total"]
        assert d["pedestrian_force"].shape == (so[b + 1] - so[b], 2)
        np.testing.assert_array_equal(d["pedestrian_force"], buf[0, so[b]:so[b + 1]])
        np.testing.assert_array_equal(d["total"], buf[1, so[b]:so[b + 1]])
    frames = np.zeros((4, 6, 7, 3), np.float32)                 # [F][K][N_total][C] of a recorded run, 3-D
    frames[2, 4, 5] = (1.0, 2.0, 3.0)
    out = split_forces(frames, so)
    assert out[2]["dynamic_obstacle_force"].shape == (4, 4, 3)
    np.testing.assert_array_equal(out[2]["dynamic_obstacle_force"][2, 2], (1.0, 2.0, 3.0))
    assert out[1]["total"].shape == (4, 0, 3)
    with pytest.raises(ValueError):
        split_forces(np.zeros((5, 7, 2), np.float32), so)          # 5 forces for a selection of 6
    with pytest.raises(ValueError):
        split_forces(np.zeros((6, 8, 2), np.float32), so)          # 8 rows for 7


def test_record_bytes_arithmetic():
    # per row and frame: 16 B of {x, y, vx, vy}, 8 B of {z, vz} when asked, 4 B per force component
    assert record_bytes(10, 3, True) == 10 * 3 * (16 + 6 * 2 * 4)
    assert record_bytes(10, 3, False, zframes=True) == 10 * 3 * (16 + 8 + 6 * 3 * 4)
    assert record_bytes(10, 3, True, forces="total") == 10 * 3 * (16 + 8)
    n = 1024 * 64
    F = n_frames(50, 1)
    assert record_bytes(n, F, True) < MAX_RECORD_BYTES           # the measured setup fits in one call
    # frames alone fit, frames and all six planar forces do not: the limit is on the two together
    assert 3_000_000 * 8 * 16 < MAX_RECORD_BYTES < record_bytes(8, 3_000_000, True)


def test_abi_version_carries_the_force_records():
    assert _lib.ABI_VERSION >= 10
    assert _lib.SINCE["sfm_batch_tick_forces"] == 10 and _lib.SINCE["sfm_batch_run_recorded_forces"] == 10
    assert "sfm_batch_tick_forces" in _lib.SYMBOLS and "sfm_batch_run_recorded_forces" in _lib.SYMBOLS
