"""Host-side tests of the batch's snapshot and restart (no GPU): ``restart_mask`` -- what it accepts and what it refuses -- and the
ABI 13 entries in header and binding."""
import os
import re

import numpy as np
import pytest

from carla_social_force_model_amd import _lib
from carla_social_force_model_amd.batch import restart_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _is_mask(m, B, ones):
    assert isinstance(m, np.ndarray) and m.dtype == np.uint8 and m.shape == (B,) and m.flags["C_CONTIGUOUS"]
    assert np.array_equal(np.nonzero(m)[0], np.asarray(sorted(ones), dtype=np.int64)) and set(m.tolist()) <= {0, 1}


def test_restart_mask_accepts():
    _is_mask(restart_mask(5), 5, range(5))                                    # None: every scene
    _is_mask(restart_mask(5, None), 5, range(5))
    _is_mask(restart_mask(5, np.array([True, False, False, True, False])), 5, [0, 3])
    _is_mask(restart_mask(3, np.zeros(3, bool)), 3, [])
    _is_mask(restart_mask(5, [1]), 5, [1])
    _is_mask(restart_mask(5, (0, 3)), 5, [0, 3])
    _is_mask(restart_mask(5, [4, 0, 4, 4, 0]), 5, [0, 4])                     # duplicates, any order
    _is_mask(restart_mask(5, []), 5, [])                                      # nobody
    _is_mask(restart_mask(5, np.array([2, 3], dtype=np.uint16)), 5, [2, 3])
    _is_mask(restart_mask(5, np.int64(2)), 5, [2])                            # one index
    _is_mask(restart_mask(1, [0]), 1, [0])
    _is_mask(restart_mask(2, [True, False]), 2, [0])                          # a list of bools is a bool mask


def test_restart_mask_refuses():
    for bad in (np.ones(4, bool), np.ones(6, bool), np.ones((5, 1), bool), np.zeros(0, bool)):
        with pytest.raises(ValueError, match="bool mask"):
            restart_mask(5, bad)
    for bad in ([5], [-1], [0, 1, 7], np.array([2**40])):
        with pytest.raises(ValueError, match=r"0 \.\. 4"):
            restart_mask(5, bad)
    for bad in ([1.0], [0.5, 2], np.array([1, 2], dtype=np.float32), ["1"], [None]):
        with pytest.raises(ValueError, match="integers"):
            restart_mask(5, bad)


def test_abi13_entry_points_are_declared():
    assert _lib.ABI_VERSION >= 13
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert int(re.search(r"#define SFM_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    for name in ("sfm_batch_snapshot", "sfm_batch_restart"):
        assert name in _lib.SYMBOLS and _lib.SINCE[name] == 13
        assert re.search(r"^int " + name + r"\(SfmBatch\* b", header, re.M), name
    assert len(_lib.SYMBOLS["sfm_batch_snapshot"][1]) == 1
    assert len(_lib.SYMBOLS["sfm_batch_restart"][1]) == 2
