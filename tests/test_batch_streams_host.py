"""CPU tests of the host side of the batch's waypoint streams and recorded runs (batch.py): the per-scene split of recorded frames,
the frame count of a recorded run, and the broadcasting and validation of set_waypoint_streams' arguments before any library call."""
import numpy as np
import pytest

from carla_social_force_model_amd import _lib
from carla_social_force_model_amd.batch import n_frames, split_frames, stream_arrays


def test_split_frames_shapes_and_order():
    scene_off = np.array([0, 3, 3, 4, 9], np.int32)
    F, C = 5, 4
    frames = np.arange(F * 9 * C, dtype=np.float32).reshape(F, 9, C)
    parts = split_frames(frames, scene_off)
    assert [p.shape for p in parts] == [(F, 3, C), (F, 0, C), (F, 1, C), (F, 5, C)]
    assert all(p.dtype == np.float32 for p in parts)
    assert np.array_equal(np.concatenate(parts, axis=1), frames)          # concatenated scene order, frame by frame
    assert np.array_equal(parts[3][2, 0], frames[2, 4])
    z = np.zeros((F, 9, 2), np.float32)
    assert [p.shape for p in split_frames(z, scene_off)] == [(F, 3, 2), (F, 0, 2), (F, 1, 2), (F, 5, 2)]
    assert [p.shape for p in split_frames(np.zeros((0, 9, 4), np.float32), scene_off)] == [(0, 3, 4), (0, 0, 4), (0, 1, 4), (0, 5, 4)]
    with pytest.raises(ValueError):
        split_frames(np.zeros((F, 8, 4), np.float32), scene_off)           # rows do not match the scenes
    with pytest.raises(ValueError):
        split_frames(np.zeros((9, 4), np.float32), scene_off)


def test_frame_count_of_a_recorded_run():
    assert n_frames(9, 4) == 3 and n_frames(8, 4) == 2 and n_frames(1, 4) == 1 and n_frames(9, 1) == 9
    assert n_frames(9, 4, max_frames=2) == 2 and n_frames(9, 4, max_frames=10) == 3 and n_frames(9, 4, max_frames=0) == 0
    assert n_frames(0, 4) == 0
    assert n_frames(-1, 4) == 0 and n_frames(4, 0) == 0 and n_frames(4, 2, max_frames=-1) == 0   # the library refuses these


def test_stream_arguments_broadcast():
    seed, side, thr = stream_arrays(3, 7, 20.0)
    assert seed.dtype == np.uint32 and side.dtype == np.float32 and thr.dtype == np.float32
    assert seed.tolist() == [7, 7, 7] and side.tolist() == [20.0] * 3 and thr.tolist() == [2.0] * 3
    assert all(a.flags["C_CONTIGUOUS"] and a.shape == (3,) for a in (seed, side, thr))
    seed, side, thr = stream_arrays(3, [1, 2, 3], [10.0], np.array([1.0, 2.5, 0.0]))
    assert seed.tolist() == [1, 2, 3] and side.tolist() == [10.0] * 3 and thr.tolist() == [1.0, 2.5, 0.0]
    seed, _, _ = stream_arrays(2, [-1, 2 ** 32 + 5], 1.0)                  # seeds mod 2^32, like SfmEngine.set_waypoint_stream
    assert seed.tolist() == [0xFFFFFFFF, 5]
    seed, _, _ = stream_arrays(1, np.uint32(0xDEADBEEF), 1.0, 3.0)
    assert seed.tolist() == [0xDEADBEEF]


@pytest.mark.parametrize("args", [
    ([1, 2], 10.0, 2.0),                 # two seeds for three scenes
    (1, [1.0, 2.0, 3.0, 4.0], 2.0),      # four sides
    (1, 10.0, np.ones((3, 1))),          # not a vector
    (1.5, 10.0, 2.0),                    # a non-integer seed
    (1, -1.0, 2.0),                      # negative side
    (1, [1.0, np.inf, 1.0], 2.0),        # infinite side
    (1, 10.0, [2.0, np.nan, 2.0]),       # NaN threshold
    (1, 10.0, -0.1),                     # negative threshold
    (1, "10", 2.0),                      # not a number
])
def test_stream_arguments_are_validated(args):
    with pytest.raises(ValueError):
        stream_arrays(3, *args)


def test_binding_declares_the_new_calls_since_abi_7():
    for name in ("sfm_batch_set_waypoint_streams", "sfm_batch_download_waypoints", "sfm_batch_run_recorded"):
        assert name in _lib.SYMBOLS and _lib.SINCE[name] == 7
    assert _lib.ABI_VERSION >= 7
