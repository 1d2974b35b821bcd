"""Host-side tests of steered pedestrians in a batch (no GPU): ``pack_steering`` -- shapes, broadcasting and every refusal -- and
the ABI 14 entries in header and binding."""
import os
import re

import numpy as np
import pytest

from carla_social_force_model_amd import _lib
from carla_social_force_model_amd.batch import (PTR_COMMANDS, PTR_STATE, PTR_ZSTATE, STEER_OFF, STEER_PREFERRED, STEER_VELOCITY,
                                                 pack_steering)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = np.array([0, 2, 2, 5], dtype=np.int32)          # three scenes of 2, 0 and 3 rows


def _is_packed(out, kinds, u):
    kd, ux, uy, uz = out
    assert kd.dtype == np.uint8 and kd.flags["C_CONTIGUOUS"] and np.array_equal(kd, kinds)
    for a, col in zip((ux, uy, uz), np.asarray(u, dtype=np.float32).T):
        assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and np.array_equal(a, col)


def test_pack_steering_shapes():
    u = np.arange(15, dtype=np.float64).reshape(5, 3) / 4
    kinds = [1, 0, 0, 2, 1]
    _is_packed(pack_steering(np.array(kinds), u, SO), kinds, u)                              # concatenated arrays
    _is_packed(pack_steering([kinds[:2], [], kinds[2:]], [u[:2], np.zeros((0, 3)), u[2:]], SO), kinds, u)      # per scene
    _is_packed(pack_steering([kinds[:2], [], kinds[2:]], [u[:2], None, u[2:]], SO), kinds, u)
    u2 = np.column_stack([u[:, :2], np.zeros(5)])
    _is_packed(pack_steering(np.array(kinds), u[:, :2], SO), kinds, u2)                       # two columns: uz = 0
    _is_packed(pack_steering([kinds[:2], [], kinds[2:]], [u[:2, :2], None, u[2:, :2]], SO), kinds, u2)
    assert (STEER_OFF, STEER_VELOCITY, STEER_PREFERRED) == (0, 1, 2) and (PTR_COMMANDS, PTR_STATE, PTR_ZSTATE) == (0, 1, 2)


def test_pack_steering_broadcasts():
    _is_packed(pack_steering(0, None, SO), [0] * 5, np.zeros((5, 3)))                        # one kind for every row, no commands
    _is_packed(pack_steering(2, np.array([0.5, -1.0]), SO), [2] * 5, [[0.5, -1.0, 0.0]] * 5)  # one command for every row
    _is_packed(pack_steering([1, 0, 2], [[1.0, 2.0, 3.0], None, [4.0, 5.0]], SO), [1, 1, 2, 2, 2],
               [[1, 2, 3], [1, 2, 3], [4, 5, 0], [4, 5, 0], [4, 5, 0]])                     # one kind and one command per scene
    kd, ux, uy, uz = pack_steering(None, np.ones((5, 2)), SO)                                 # the commands alone
    assert kd is None and np.array_equal(ux, np.ones(5, np.float32)) and not uz.any()
    kd, ux, uy, uz = pack_steering(1, None, np.array([0, 0]))                                 # a batch without rows
    assert kd.shape == ux.shape == uy.shape == uz.shape == (0,)
    # a row that is not steered may hold anything
    u = np.full((5, 3), np.nan)
    u[4] = 1.0
    assert np.array_equal(pack_steering(np.array([0, 0, 0, 0, 1]), u, SO)[0], [0, 0, 0, 0, 1])


def test_pack_steering_refuses():
    with pytest.raises(ValueError, match="2 entries of kinds for 3 scenes"):
        pack_steering([[1, 0], [0, 0, 0]], None, SO)
    with pytest.raises(ValueError, match="scene 2: kinds of shape"):
        pack_steering([[1, 0], [], [0, 0]], None, SO)
    with pytest.raises(ValueError, match=r"kinds of shape \(4,\) for 5 rows"):
        pack_steering(np.zeros(4), None, SO)
    for bad in (3, -1, 0.5, np.array([0, 1, 2, 3, 0]), [[0, 1], [], [2, 2, 7]]):
        with pytest.raises(ValueError, match="kinds must hold 0"):
            pack_steering(bad, None, SO)
    with pytest.raises(ValueError, match="scene 0: commands of shape"):
        pack_steering(0, [np.zeros((3, 2)), None, np.zeros((3, 2))], SO)
    with pytest.raises(ValueError, match="commands of shape"):
        pack_steering(0, np.zeros((5, 4)), SO)
    with pytest.raises(ValueError, match="commands of shape"):
        pack_steering(0, np.zeros((4, 2)), SO)
    for val in (np.nan, np.inf, -np.inf, 1e39):                                               # 1e39 is not finite in float32
        for col in range(3):
            u = np.zeros((5, 3))
            u[3, col] = val
            with pytest.raises(ValueError, match="row 3: the command of a steered row must be finite"):
                pack_steering(np.array([0, 0, 0, 2, 0]), u, SO)
            with pytest.raises(ValueError, match="row 3"):
                pack_steering(None, u, SO)
            assert pack_steering(np.array([1, 1, 1, 0, 2]), u, SO)[0][3] == 0                 # ... unless the row is not steered


def test_abi14_entry_points_are_declared():
    assert _lib.ABI_VERSION >= 14
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert int(re.search(r"#define SFM_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    for name in ("sfm_batch_set_steering", "sfm_batch_set_commands", "sfm_batch_download_steering", "sfm_batch_device_ptr"):
        assert name in _lib.SYMBOLS and _lib.SINCE[name] == 14
        assert re.search(r"^(int|void\*) " + name + r"\(SfmBatch\* b", header, re.M), name
    assert [len(_lib.SYMBOLS[n][1]) for n in ("sfm_batch_set_steering", "sfm_batch_set_commands", "sfm_batch_download_steering",
                                              "sfm_batch_device_ptr")] == [5, 4, 5, 3]
    for k, name in enumerate(("SFM_BATCH_PTR_COMMANDS", "SFM_BATCH_PTR_STATE", "SFM_BATCH_PTR_ZSTATE")):
        assert re.search(r"#define " + name + r" " + str(k) + r"\b", header), name
