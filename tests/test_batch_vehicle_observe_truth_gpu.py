"""GPU tests that pin sfm_batch_vehicle_observe_kernel (SfmBatch.vehicle_observations) to a float64 statement of the record and to
designed exact cases written down by hand (_vehicle_observe_cases.py), neither of which goes through the host twin -- and, beside
them, to the twin bit for bit at sizes the older file does not reach: 1024 rows (the LDS array full), 129 rows (a third lane pass),
70 vehicles in a scene (a wave owns 17 or 18, the other_d2 search makes two lane passes).  Also: scene independence, the forms of
the mask, that an observed record is written whole and nothing else is written, restarts.
Run on the MI355X box with  python -m pytest tests -m gpu."""
from functools import lru_cache

import numpy as np
import pytest

import _driving_cases as D
import _vehicle_observe_cases as T
import test_batch_vehicles_gpu as V
from carla_social_force_model_amd import observe

pytestmark = pytest.mark.gpu

KS = (1, 4, 16)
EVERY = tuple(range(len(T.SIZES)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _batch(k, frame, spread=False, which=EVERY, mask="fixture"):
    """A batch of the fixture's scenes ``which``, tracked, driven and observed; the twin started.  ``mask``: "fixture", None, or a
    list per scene."""
    pick = lambda xs: [xs[s] for s in which]
    scenes, cfgs, tracks, fmask, goals, kinds, cmds = (pick(xs) for xs in T.made(spread, start=False))
    mask = fmask if isinstance(mask, str) else mask
    b = V._batch(scenes, cfgs, pick(T.DTS))
    try:
        b.set_vehicle_tracks(tracks)
        b.set_vehicle_driving(kinds, cmds)
        b.set_vehicle_observation(k, pick(T.RANGES), frame, goals=goals, mask=mask)
    except Exception:
        b.close()
        raise
    D.start_twin(scenes, tracks)
    return b, scenes, tracks, mask, goals, kinds, cmds


def _drive(b, scenes, kinds, cmds, tracks, ticks, which=EVERY):
    b.run(ticks)
    for t in range(ticks):
        D.drive_twin(scenes, kinds, cmds, [T.DTS[s] for s in which], tracks, t + 1)


def _twin(scenes, k, frame, mask, goals, state, which=EVERY):
    return [observe.observe_vehicles_scene(sc, k, T.RANGES[which[i]], frame, goals=goals[i], mask=None if mask is None else mask[i],
                                           state=state[i]) for i, sc in enumerate(scenes)]


@lru_cache(maxsize=None)
def _planar_upload(k, frame):
    b, *_ = _batch(k, frame)
    try:
        return b.vehicle_observations()
    finally:
        b.close()


@pytest.mark.parametrize("spread", [False, True], ids=["planar", "3-D"])
@pytest.mark.parametrize("frame", [0, 1], ids=["world", "heading"])
@pytest.mark.parametrize("k", KS)
def test_the_device_lies_inside_the_float64_envelope(k, frame, spread):
    """T.check on what the device returns, not through the twin: at the upload and after 3 driven ticks, with the device's own state
    and vehicles fed to the float64 statement.  A 3-D batch reads at the upload what the planar batch reads, bit for bit."""
    b, scenes, tracks, mask, goals, kinds, cmds = _batch(k, frame, spread)
    try:
        assert b.planar != spread
        compared = left_out = 0
        for round_ in range(2):
            got, state, veh = b.vehicle_observations(), b.state(), b.dynamic_obstacles()
            if spread and round_ == 0:
                assert all(np.array_equal(_bits(g), _bits(p)) for g, p in zip(got, _planar_upload(k, frame)))
            bad = []
            for s, sc in enumerate(scenes):
                V._same_vehicles(veh[s], sc, f"round {round_}, scene {s}")             # the moved vehicles are the device's
                res = T.check(got[s], sc, k, T.RANGES[s], frame, goals=goals[s], mask=mask[s], state=state[s], vehicles=veh[s])
                compared, left_out = compared + res["compared"], left_out + res["left_out"]
                bad += [f"round {round_}, scene {s}, {x}" for x in res["bad"]]
            assert not bad, bad[:8]
            if round_ == 0:
                _drive(b, scenes, kinds, cmds, tracks, 3)
        assert compared + left_out == 2 * sum(T.COUNTS) and left_out <= 0.01 * 2 * sum(T.COUNTS), (compared, left_out)
    finally:
        b.close()


@pytest.mark.parametrize("frame", [0, 1], ids=["world", "heading"])
@pytest.mark.parametrize("k", KS)
def test_the_device_equals_the_twin_bit_for_bit(k, frame):
    """The same fixture against observe.observe_vehicles_scene, at the upload and after 3 driven ticks."""
    b, scenes, tracks, mask, goals, kinds, cmds = _batch(k, frame)
    try:
        for round_ in range(2):
            got, state = b.vehicle_observations(), b.state()
            for s, want in enumerate(_twin(scenes, k, frame, mask, goals, state)):
                assert got[s].shape == want.shape and np.array_equal(got[s], want, equal_nan=True), \
                    f"round {round_}: scene {s}, vehicles {np.flatnonzero((got[s] != want).any(axis=1))}"
            if round_ == 0:
                _drive(b, scenes, kinds, cmds, tracks, 3)
    finally:
        b.close()


def _device_on(sc, k, R, tracks):
    b = V._batch([sc], [V._config(0, V.ALL)], [0.05])
    try:
        if tracks is not None:
            b.set_vehicle_tracks([tracks])
        b.set_vehicle_observation(k, [float(R)], 0)
        return b.vehicle_observations()[0]
    finally:
        b.close()


@pytest.mark.parametrize("kind", [None, 0, 1], ids=["rows and distances", "border points", "static points"])
def test_designed_cases(kind):
    """The expected neighbours and points are stated literally in _vehicle_observe_cases.designed; the device equals them bit for
    bit: same-lane and cross-lane ties, more tied rows than slots, a tie that straddles the last slot, rows and points at exactly R
    and one fp32 step inside it, equidistant points in every arrangement of lanes and polylines, NaN border points (SfmBatch.upload
    accepts them), the two distances without anything to measure."""
    for name, sc, k, R, want, tracks in T.designed(kind):
        got = _device_on(sc, k, R, tracks)
        assert T.same_bits(got[0], want), (name, got[0], want)
        if name == "another vehicle":
            assert not got[1].any() and got[2, 9] == 25.0 and got[2, 6] == 1.0
        else:
            assert not got[1:].any(), name


def test_a_scene_reads_the_same_alone_and_anywhere_in_a_batch():
    """The 70-vehicle scene and the 1024-row scene: in the fixture's batch, each alone, and at other indices of a smaller batch."""
    k, frame = 16, 1
    full = _planar_upload(k, frame)
    for which in ((8,), (7,), (8, 1, 7)):
        b, *_ = _batch(k, frame, which=which)
        try:
            got = b.vehicle_observations()
        finally:
            b.close()
        for i, s in enumerate(which):
            assert np.array_equal(_bits(got[i]), _bits(full[s])), (which, s)


def test_the_forms_of_the_mask():
    """mask = None and all ones agree bit for bit; all zeros for one scene reads zeros there and changes no other scene's record."""
    k, frame = 4, 0
    ones = [np.ones(m, np.uint8) for m in T.COUNTS]
    out = [np.zeros(m, np.uint8) if s == 8 else np.ones(m, np.uint8) for s, m in enumerate(T.COUNTS)]
    recs = []
    for mask in (None, ones, out):
        b, *_ = _batch(k, frame, mask=mask)
        try:
            recs.append(b.vehicle_observations())
        finally:
            b.close()
    assert (recs[0][8][:, 6] == 1.0).sum() == 69
    for s in EVERY:
        assert np.array_equal(_bits(recs[0][s]), _bits(recs[1][s])), s
        if s == 8:
            assert not _bits(recs[2][s]).any()
        else:
            assert np.array_equal(_bits(recs[0][s]), _bits(recs[2][s])), s


def test_an_observed_record_is_written_whole_and_nothing_else_is_written():
    """The buffer filled with NaN through vehicle_observation_tensor(): after a launch the records of observed present vehicles hold
    no NaN (empty slots included), those of observed absent vehicles are zeros, those of masked-out vehicles still hold the fill.
    Then the crowd of one scene moves away: the slots its vehicles had filled read zeros."""
    import torch
    k, frame, s = 4, 1, 6
    b, scenes, tracks, mask, goals, kinds, cmds = _batch(k, frame)
    try:
        io = b._dyn[0]
        buf = b.vehicle_observation_tensor()
        assert tuple(buf.shape) == (sum(T.COUNTS), 16 + 4 * k)
        torch.cuda.synchronize()
        buf.fill_(float("nan"))
        torch.cuda.synchronize()
        b.observe_vehicles()
        got = b.vehicle_observations()                                     # (a second launch and the download: it synchronises)
        seen = dict(present=0, absent=0, masked=0)
        for q, sc in enumerate(scenes):
            for v, (c, _) in enumerate(sc["dynamic_obstacles"]):
                r = got[q][v]
                if not mask[q][v]:
                    assert np.isnan(r).all(), (q, v)
                    seen["masked"] += 1
                elif not np.isfinite(c).all():
                    assert not _bits(r).any(), (q, v)
                    seen["absent"] += 1
                else:
                    assert not np.isnan(r).any() and r[6] == 1.0 and not r[16 + 4 * int(r[7]):].any(), (q, v)
                    seen["present"] += 1
        assert seen == dict(present=sum(int(m.sum()) for m in mask) - 1, absent=1, masked=sum(int((m == 0).sum()) for m in mask)), seen
        assert np.array_equal(_bits(buf.cpu().numpy()), _bits(np.concatenate(got))) and int(io[-1]) == sum(T.COUNTS)
        before = got[s]
        assert (before[1:, 7] > 0).all() and (before[1:, 7] == k).any()   # (vehicle 0 of this scene is masked out)
        so = b.scene_off
        st = b.state_tensor()
        st[int(so[s]):int(so[s + 1]), 0] += 1000.0                         # the crowd of scene s, a kilometre away
        torch.cuda.synchronize()
        after = b.vehicle_observations()
        assert np.isnan(after[s][0]).all()
        assert (after[s][1:, 7] == 0).all() and not after[s][1:, 16:].any() and (after[s][1:, 8] > 1.0e5).all()
        for q in EVERY:
            if q != s:
                assert np.array_equal(_bits(after[q]), _bits(got[q])), q
        rec = after[s].copy()
        rec[0] = 0.0                                                       # (what a buffer that nobody filled would hold there)
        res = T.check(rec, scenes[s], k, T.RANGES[s], frame, goals=goals[s], mask=mask[s], state=b.state()[s])
        assert not res["bad"] and res["compared"] == T.COUNTS[s], res
    finally:
        b.close()


def test_restarted_scenes_read_what_they_read_at_the_snapshot():
    """Snapshot, observe, 5 driven ticks, restart by host mask (scenes 1 and 8) and by a mask on the device (3 and 7), observe: the
    restarted scenes read the snapshot's records bit for bit, the others what the twin says for their moved state."""
    import torch
    k, frame = 4, 1
    b, scenes, tracks, mask, goals, kinds, cmds = _batch(k, frame)
    try:
        b.snapshot()
        first = b.vehicle_observations()
        _drive(b, scenes, kinds, cmds, tracks, 5)
        moved = b.vehicle_observations()
        assert all(not np.array_equal(_bits(moved[s]), _bits(first[s])) for s in (1, 3, 7, 8))
        b.restart([1, 8])
        dev = torch.zeros(len(EVERY), dtype=torch.uint8, device="cuda")
        dev[3] = dev[7] = 1
        torch.cuda.synchronize()
        b.restart_device(dev)
        got, state = b.vehicle_observations(), b.state()
        want = _twin(scenes, k, frame, mask, goals, state)
        for s in EVERY:
            if s in (1, 3, 7, 8):
                assert np.array_equal(_bits(got[s]), _bits(first[s])), s
            else:
                assert np.array_equal(got[s], want[s], equal_nan=True) and np.array_equal(_bits(got[s]), _bits(moved[s])), s
    finally:
        b.close()
