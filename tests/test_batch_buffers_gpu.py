"""GPU test of the one lookup behind the batch's device pointers (sfm_batch_device_ptr for every ``which``, and
sfm_batch_observation_ptr): before a feature is set a null pointer, 0 bytes and the library's exact message; once it is set the
pointer and the byte count (null and 0 where the batch has no rows, or a planar batch no {z, vz}); after the next upload off again.
On a planar batch of 3 and 0 rows, the same batch in 3-D, and a batch whose scenes are all empty.  And end_step with the auto
restart refuses for the missing snapshot before it launches anything.  Nothing but refusals and plain queries.  Run on the MI355X box
with  python -m pytest tests -m gpu."""
import ctypes as C

import numpy as np
import pytest

from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd._lib import SfmLibraryError
from carla_social_force_model_amd.batch import PTR_COMMANDS, PTR_DONE, PTR_EPISODES, PTR_SCAN, PTR_STATE, PTR_ZSTATE, SfmBatch
from carla_social_force_model_amd.config import default_sfm_config

pytestmark = pytest.mark.gpu

PTR_OBS = "observations"                 # sfm_batch_observation_ptr, beside the six values of `which`
NO_STATE = "sfm_batch_upload_state has not been called"
STEERING_OFF = "steering is off: call sfm_batch_set_steering first (sfm_batch_upload_state drops it)"
OBSERVATIONS_OFF = "observations are off: call sfm_batch_set_observation first (sfm_batch_upload_state drops them)"
EPISODES_OFF = ("episodes are off: call sfm_batch_set_episodes first (sfm_batch_upload_state drops them), so which = "
                "SFM_BATCH_PTR_EPISODES / _DONE has no buffer")
SCANS_OFF = "scans are off: call sfm_batch_set_scan first (sfm_batch_upload_state drops them), so which = SFM_BATCH_PTR_SCAN has no buffer"
BAD_WHICH = "which must be SFM_BATCH_PTR_COMMANDS, _STATE, _ZSTATE, _EPISODES, _DONE or _SCAN"
NO_SNAPSHOT = ("the batch has no snapshot: call sfm_batch_snapshot first (sfm_batch_upload_state and the calls that set vehicles, "
               "modes, a spawn schedule or tracks drop it)")
K, R = 1, 1


def _scene(n, z3):
    i = np.arange(n, dtype=np.float64)
    loc = np.column_stack([2.0 * i, 0.5 * i, 0.25 * i if z3 else np.zeros(n)])
    return {"loc": loc, "vel": np.column_stack([np.full(n, 0.5), np.zeros(n), np.full(n, 0.1 if z3 else 0.0)]),
            "waypoint": loc + np.array([10.0, 0.0, 0.0]), "target_speed": np.full(n, 1.3)}


def _query(b, which):
    """(pointer or None, bytes, the batch's last error after the call)"""
    nbytes = C.c_int64(-1)
    if which == PTR_OBS:
        ptr = b._lib.sfm_batch_observation_ptr(b._b, C.byref(nbytes))
    else:
        ptr = b._lib.sfm_batch_device_ptr(b._b, which, C.byref(nbytes))
    return ptr, nbytes.value, b._lib.sfm_batch_last_error(b._b).decode()


def _refused(b, which, message):
    assert _query(b, which) == (None, 0, message), which


def _sensors_off(b, n, z3):
    """after an upload and before any sensor is set: the state is there, everything else is off"""
    _refused(b, PTR_COMMANDS, STEERING_OFF)
    _refused(b, PTR_EPISODES, EPISODES_OFF)
    _refused(b, PTR_DONE, EPISODES_OFF)
    _refused(b, PTR_SCAN, SCANS_OFF)
    _refused(b, PTR_OBS, OBSERVATIONS_OFF)
    _answered(b, PTR_STATE, 16 * n, OBSERVATIONS_OFF)
    _answered(b, PTR_ZSTATE, 8 * n if z3 else 0, OBSERVATIONS_OFF)


def _answered(b, which, nbytes, last_error):
    """a buffer of nbytes (0: a null pointer, and no refusal -- the last error is still the one before)"""
    ptr, got, err = _query(b, which)
    assert got == nbytes and (ptr is not None) == (nbytes > 0) and err == last_error, (which, ptr, got, err)


@pytest.mark.parametrize("sizes,z3", [((3, 0), False), ((3, 0), True), ((0, 0), False)])
def test_every_device_pointer_before_and_after_its_feature_is_set(sizes, z3):
    B, n = len(sizes), sum(sizes)
    scenes = [_scene(m, z3) for m in sizes]
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), 0.05, B=B)
    try:
        for which in (PTR_COMMANDS, PTR_STATE, PTR_ZSTATE):            # before any upload
            _refused(b, which, NO_STATE)
        _refused(b, PTR_EPISODES, EPISODES_OFF)
        _refused(b, PTR_OBS, OBSERVATIONS_OFF)
        b.upload(scenes)
        assert b.planar == (not z3 or n == 0)
        z3 = not b.planar
        for which in (-1, 6):
            _refused(b, which, BAD_WHICH)
        _sensors_off(b, n, z3)

        b.set_steering(0)
        b.set_observation(K, 5.0)
        b.set_episodes([0 if m else -1 for m in sizes], 1.0, 0.3, 1.0, 0)
        b.set_scan(10.0, 0.3, R=R)
        last = OBSERVATIONS_OFF                                        # (no refusal since: nothing below overwrites it)
        _answered(b, PTR_COMMANDS, 16 * n, last)
        _answered(b, PTR_STATE, 16 * n, last)
        _answered(b, PTR_ZSTATE, 8 * n if z3 else 0, last)
        _answered(b, PTR_EPISODES, 32 * B, last)
        _answered(b, PTR_DONE, B, last)
        _answered(b, PTR_SCAN, 4 * n * 2 * R, last)
        _answered(b, PTR_OBS, 4 * n * (16 + 4 * K), last)
        assert b._lib.sfm_batch_device_ptr(b._b, PTR_DONE, None) is not None      # bytes may be NULL
        for which in (-1, 6):
            _refused(b, which, BAD_WHICH)

        b.upload(scenes)                                               # drops every one of them
        _sensors_off(b, n, z3)
    finally:
        b.close()


def test_auto_restart_without_a_snapshot_is_refused_before_anything_is_launched():
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), 0.05, B=2)
    try:
        b.upload([_scene(3, False), _scene(0, False)])
        b.set_episodes([0, -1], 1.0, 0.3, 1.0, 0)
        assert not b.has_snapshot
        with pytest.raises(SfmLibraryError) as e:
            b.end_step(auto_restart=True)
        assert str(e.value) == f"sfm_batch_end_step failed (-3): {NO_SNAPSHOT}"
        rec, done = b.episodes()                                       # as set_episodes zero-filled them: no end_step has run
        assert not rec.any() and not done.any()
        b.end_step()                                                   # (the plain end_step does run: age 1)
        rec, done = b.episodes()
        assert rec[0, 2] == 1.0 and rec[1, 2] == 1.0
    finally:
        b.close()
