"""GPU tests of what keeps and what drops the row episodes (sfm_batch_set_row_episodes), call by call.

The header says: "sfm_batch_upload_state drops the row episodes; every other call keeps them, and they keep the snapshot".  The drop
table of tests/_lifecycle_cases.py has no rows for the row episodes (they live in the episodes' block of struct SfmBatch, as its
second half, so the table's guard over the members of the struct does not ask for one); until it has, this file holds that sentence
for EVERY call of the table, on every set-up the table makes the call on: the row episodes are set on generation A with everything
else of the set-up, evaluated once, the call is made, and the record, mask and per-row state read back as before -- or, after an
upload, the getter and the library itself say that row episodes are off.  Both halves of the block are held apart: switching the
scene episodes off or setting them again keeps the row episodes, and the reverse.  Run on the MI355X box with
python -m pytest tests -m gpu."""
import numpy as np
import pytest

import _lifecycle_cases as LC
from carla_social_force_model_amd._lib import SfmLibraryError
from carla_social_force_model_amd.batch import SfmBatch

pytestmark = pytest.mark.gpu

SFM_ERR_STATE = -3
RADII = dict(goal_radius=3.0, ped_radius=0.9, veh_radius=1.5, max_steps=2)


def _new_batch():
    import torch
    b = SfmBatch(LC.configs(), list(LC.DTS))
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
    except Exception:
        b.close()
        raise
    return b


def _setup(b, setup):
    """Generation A with everything of the set-up (tests/test_lifecycle_gpu.py's), then the row episodes, evaluated once."""
    c = LC.crowd(setup if setup in LC.PROFILES else "policy", "A")
    LC.set_everything(b, c)
    if setup not in LC.PROFILES:
        b.set_routes(None, None, None)
        b.set_spawns(c["scheds"] if setup == "spawns" else [None] * len(LC.DTS))
        b.snapshot()
    n = int(b.scene_off[-1])
    b.set_row_episodes(np.arange(n) % 2 == 0, **RADII)
    assert b.has_snapshot                                              # setting row episodes keeps the snapshot
    b.end_row_step()
    return c


def _same(u, v):
    return all(a.shape == c.shape and a.tobytes() == c.tobytes() for a, c in zip(u, v))


def _assert_rows_gone(b):
    with pytest.raises(SfmLibraryError, match="row episodes are off"):
        b.row_episodes()
    assert b._lib.sfm_batch_end_row_step(b._b, 0) == SFM_ERR_STATE
    assert b._lib.sfm_batch_download_row_episodes(b._b, None, None, None, None) == SFM_ERR_STATE
    assert "row episodes are off" in b._lib.sfm_batch_last_error(b._b).decode()


@pytest.mark.parametrize("call,setup", [(call, setup) for call in LC.CALLS for setup in LC.SETUPS[call]])
def test_every_call_of_the_drop_table(call, setup):
    b = _new_batch()
    try:
        c = _setup(b, setup)
        was = b.row_episodes()
        assert was[1].any() or was[0][:, 2].any()                      # (the evaluation left something to keep)
        LC.CALLS[call][1](b, c)
        if call == "upload":
            assert not b.has_row_episodes
            _assert_rows_gone(b)
            b.set_row_episodes(True, **RADII)                          # ... and they can be set again on the new crowd
            b.end_row_step()
            assert (b.row_episodes()[2] == 1).all()
        else:
            assert b.has_row_episodes and _same(b.row_episodes(), was), f"{call} keeps the row episodes"
            b.end_row_step()                                           # ... and they go on: the ages count up
            assert np.array_equal(b.row_episodes()[2], was[2] + (np.arange(was[2].shape[0]) % 2 == 0))
    finally:
        b.close()


def test_the_two_halves_of_the_episodes_are_set_and_dropped_apart():
    b = _new_batch()
    try:
        _setup(b, "policy")
        b.end_step()
        rows, scene = b.row_episodes(), b.episodes()
        b.set_row_episodes(None)                                        # the row episodes off: the scene episodes stay
        _assert_rows_gone(b)
        assert _same(b.episodes(), scene) and b.has_snapshot
        n = int(b.scene_off[-1])
        b.set_row_episodes(np.arange(n) % 2 == 0, **RADII)
        b.end_row_step()
        rows = b.row_episodes()
        b.set_episodes([-1 if k == 0 else 0 for k in np.diff(b.scene_off)], goal_radius=1.0)                              # the scene episodes set again: the row episodes stay
        assert _same(b.row_episodes(), rows)
        b.set_episodes(None)                                            # ... and off
        assert _same(b.row_episodes(), rows)
        with pytest.raises(SfmLibraryError, match="episodes are off"):
            b.episodes()
        b.restart()                                                     # the snapshot is still there; the restart starts the rows over
        assert not b.row_episodes()[2].any()
    finally:
        b.close()
