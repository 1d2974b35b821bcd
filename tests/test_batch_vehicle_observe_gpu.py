"""GPU tests of the batch's vehicle observations (sfm_batch_set_vehicle_observation, sfm_batch_observe_vehicles,
sfm_batch_download_vehicle_observations; SfmBatch.set_vehicle_observation / observe_vehicles / vehicle_observations): the record
against the host twin observe.observe_vehicles_scene bit for bit in both frames, at the upload and after driven ticks, and that
observing changes nothing a tick reads.  Run on the MI355X box with  python -m pytest tests -m gpu."""
import copy
from functools import lru_cache

import numpy as np
import pytest

import _driving_cases as D
import test_batch_tracks_gpu as TR
import test_batch_vehicles_gpu as V
from carla_social_force_model_amd import observe
from carla_social_force_model_amd.batch import SfmBatch

pytestmark = pytest.mark.gpu

SIZES, COUNTS = (0, 1, 63, 64, 65, 257), (2, 1, 3, 5, 2, 4)
RANGES = [4.0, 6.0, 5.0, 5.0, 3.0, 8.0]
DTS = [0.05, 0.04, 0.02, 0.05, 0.03, 0.05]


@lru_cache(maxsize=None)
def _made():
    scenes = [V._scene(n, 3100 + k, m) for k, (n, m) in enumerate(zip(SIZES, COUNTS))]
    scenes[2]["borders"], scenes[2]["border_centers"], scenes[2]["border_lengths"] = [], np.zeros((0, 2)), np.zeros(0)
    scenes[2]["static_obstacles"] = []                                     # a scene without borders or static obstacles
    # exact (d2, j) ties: rows mirrored about vehicle 0 of scene 3, whose centre has integer coordinates
    c = np.array([6.0, 5.0])
    sc = scenes[3]
    sc["dynamic_obstacles"][0] = (c, sc["dynamic_obstacles"][0][1])
    V._restart_twin(sc)
    for j, (dx, dy) in enumerate(((1.5, 0.5), (-1.5, 0.5), (0.5, -1.5), (1.5, -0.5), (-0.5, 1.5), (0.25, 0.0), (-0.25, 0.0))):
        sc["loc"][10 + 3 * j, :2] = c + (dx, dy)
    for scn, rows in ((scenes[3], (0, 7, 63)), (scenes[5], (64, 200, 256)), (scenes[1], (0,))):    # despawned rows: parked far away
        for i in rows:
            scn["loc"][i, :2] = (3.0e15 + 1.0e12 * (i + 1), -3.0e15)
            scn["vel"][i] = 0.0
    rng = np.random.default_rng(5)
    tracks = [None] * 6
    tracks[4] = [None, TR._track(rng, 5, 40, TR._mid(scenes[4]))]          # absent until tick 40
    mask = [[1, 1], [1], [1, 0, 1], [1, 1, 1, 0, 1], [1, 1], [0, 1, 1, 1]]
    goals = [rng.uniform(0.0, 12.0, (m, 2)) for m in COUNTS]
    kinds = [[2, 1], [0], [2, 0, 1], [1, 2, 0, 2, 0], [2, 1], [0, 2, 2, 1]]
    cmds = [np.column_stack((rng.uniform(-1.4, 1.4, m), np.cos(rng.uniform(-0.1, 0.1, m)), rng.uniform(-0.1, 0.1, m))).astype(np.float32)
            for m in COUNTS]
    cfgs = [V._config(k, V.ALL) for k in range(6)]
    return scenes, cfgs, tracks, mask, goals, kinds, cmds


def _batch(k, frame):
    scenes, cfgs, tracks, mask, goals, kinds, cmds = copy.deepcopy(_made())
    b = V._batch(scenes, cfgs, DTS)
    try:
        b.set_vehicle_tracks(tracks)
        b.set_vehicle_driving(kinds, cmds)
        b.set_vehicle_observation(k, RANGES, frame, goals=goals, mask=mask)
    except Exception:
        b.close()
        raise
    D.start_twin(scenes, tracks)
    return b, scenes, tracks, mask, goals, kinds, cmds


def _check(b, scenes, k, frame, mask, goals, what):
    got, state = b.vehicle_observations(), b.state()
    seen = dict(ties=0, empty=0, full=0)
    for s, sc in enumerate(scenes):
        want = observe.observe_vehicles_scene(sc, k, RANGES[s], frame, goals=goals[s], mask=mask[s], state=state[s])
        assert got[s].shape == want.shape and np.array_equal(got[s], want, equal_nan=True), \
            f"{what}: scene {s}, vehicles {np.flatnonzero((got[s] != want).any(axis=1))}"
        seen["empty"] += int(((want[:, 6] == 1) & (want[:, 7] < k)).sum())
        seen["full"] += int((want[:, 7] == k).sum())
    return got, seen


@pytest.mark.parametrize("frame", [0, 1], ids=["world", "heading"])
@pytest.mark.parametrize("k", [1, 4, 16])
def test_vehicle_observations_equal_the_twin(k, frame):
    """Scenes of 0, 1, 63, 64, 65 and 257 rows (the lane strides wrap), k = 1, 4, 16, both frames: every record bit for bit, at
    the upload and after 3 driven ticks; a masked-out and an absent vehicle read zeros, a scene without borders or statics +inf and
    zeros, despawned rows never appear, exact ties go to the lower row."""
    b, scenes, tracks, mask, goals, kinds, cmds = _batch(k, frame)
    try:
        for round_ in range(2):
            got, seen = _check(b, scenes, k, frame, mask, goals, f"round {round_}")
            assert not got[2][1].any() and not got[3][3].any() and not got[5][0].any()        # masked out
            assert not got[4][1].any() and got[4][0][6] == 1.0                                # absent; its neighbour is there
            assert np.isposinf(got[0][:, 8]).all() and (got[0][:, 7] == 0).all() and (got[0][:, 6] == 1).all()   # no rows at all
            assert (got[2][[0, 2], 14] == 0).all() and not got[2][[0, 2], 10:14].any()        # no borders, no statics
            assert np.isfinite(got[3][0, 9]) and np.isposinf(got[1][0, 9])                    # other vehicles / none
            assert seen["full"] > 0 and (k == 1 or seen["empty"] > 0)
            for s, sc in enumerate(scenes):                                                   # a ghost is nobody's neighbour
                assert np.abs(got[s][:, 16::4]).max(initial=0.0) < 1.0e6
            if round_ == 0:
                if frame == 0 and k >= 4:                                                     # the mirrored rows: (d2, j) order
                    slots = got[3][0][16:16 + 4 * k].reshape(k, 4)[:, :2]
                    assert np.array_equal(slots[:2], np.float32([[0.25, 0.0], [-0.25, 0.0]]))   # rows 25 and 28, d2 = 0.0625 both
                    if k == 16:                                                               # rows 10 and 13, d2 = 2.5 both
                        tied = [int(np.flatnonzero((slots == np.float32(p)).all(axis=1))[0]) for p in ((1.5, 0.5), (-1.5, 0.5))]
                        assert tied[1] == tied[0] + 1
                b.run(3)
                for t in range(3):
                    D.drive_twin(scenes, kinds, cmds, DTS, tracks, t + 1)
    finally:
        b.close()


def test_observing_changes_nothing_a_tick_reads():
    """State and vehicles after run(5) are bit-equal with and without observe_vehicles() calls in between."""
    a, *_ = _batch(4, 1)
    b, *_ = _batch(4, 1)
    try:
        a.run(5)
        for _ in range(5):
            b.observe_vehicles()
            b.run(1)
            b.observe_vehicles()
        V._assert_same(V._everything(a), V._everything(b), "with and without observing")
        for x, y in zip(a.vehicle_driving(), b.vehicle_driving()):
            assert all(np.array_equal(u, v) for u, v in zip(x, y))
        oa, ob = a.vehicle_observations(), b.vehicle_observations()
        assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(oa, ob))
    finally:
        a.close()
        b.close()
