"""GPU tests of the batch's restart noise (sfm_batch_set_restart_noise; SfmBatch.set_restart_noise / restart_noise).

The oracle is the NumPy twin ``reset.resample_scene``, and every comparison is bitwise: after a snapshot and a few ticks, three
consecutive restarts (e = 0, 1, 2) of the crowd of tests/_reset_cases.py -- six scenes of 1, 2, 63, 65, 300 and 1 024 rows -- through
each of the three restart paths must leave exactly the twin's positions, goals, first ticks (seen through presence, centres and
rings), vehicles and counters in the chosen scenes and touch nothing in the others.  tests/test_batch_reset_host.py shows on the CPU
that this crowd rejects under every condition, places rows in late rounds and has fallbacks.  Run on the MI355X box with
python -m pytest tests -m gpu."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import _reset_cases as RC
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd._lib import SfmLibraryError
from carla_social_force_model_amd.batch import SfmBatch, pack_restart_noise
from carla_social_force_model_amd.config import default_sfm_config

pytestmark = pytest.mark.gpu

ALL = tuple(range(len(RC.SIZES)))
K0, K1 = 2, 3                    # ticks before the snapshot, ticks between the snapshot and the restarts
SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3
CHOSEN = {"host": (0, 1, 2, 3, 5), "device": (0, 1, 3, 4, 5), "end_step": (1, 2, 3, 4, 5)}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32)).view(np.uint32)


def _noise(b, which):
    a = RC.noise_args()
    dl = np.concatenate([np.array([RC.DELAY, 3], np.int32) if RC.scenes()[k]["dynamic_obstacles"] else np.zeros(0, np.int32) for k in which])
    b.set_restart_noise(a["seeds"][list(which)], [a["pos_box"][k] for k in which], [a["goal_box"][k] for k in which], a["min_gap"],
                        a["point_gap"], a["tries"], dl)


def _build(which=ALL, noise=True, scenes=None, tracks=None):
    scenes = [RC.scenes()[k] for k in which] if scenes is None else scenes
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), [RC.DTS[k] for k in which])
    try:
        b.upload(scenes, device_vehicles=True)
        b.set_vehicle_tracks([RC.tracks()[k] for k in which] if tracks is None else tracks)
        if noise:
            _noise(b, which)
    except Exception:
        b.close()
        raise
    return b


def _read(b):
    """Everything a noisy restart can change, per scene."""
    tick, present = b.vehicle_tracks()
    resets, fallbacks = b.restart_noise() if b.has_restart_noise else (np.zeros(b.B, np.uint32),) * 2
    return [{"loc": _bits(loc), "vel": _bits(vel), "wp": _bits(wp), "draws": d, "ctr": [_bits(c) for c, _ in veh],
             "ring": [_bits(r) for _, r in veh], "present": p, "resets": resets[k], "fallbacks": fallbacks[k]}
            for k, ((loc, vel), (wp, d), veh, p) in enumerate(zip(b.state(), b.waypoints(), b.dynamic_obstacles(), present))]


def _same(got, want, what):
    assert got.keys() == want.keys()
    for name, u in got.items():
        v = want[name]
        if isinstance(u, list):
            assert len(u) == len(v) and all(np.array_equal(p, q) for p, q in zip(u, v)), f"{what}: {name}"
        else:
            assert np.array_equal(u, v), f"{what}: {name}"


def _to_snapshot(b):
    """K0 ticks, the snapshot, K1 ticks; returns what the snapshot holds, read before the K1 ticks."""
    b.run(K0)
    b.snapshot()
    held = (b.state(), b.waypoints(), b.dynamic_obstacles())
    b.run(K1)
    return held


@lru_cache(maxsize=None)
def _held():
    """The snapshot of the whole crowd (ticks are deterministic: every batch built alike holds the same).  Computed once."""
    b = _build(noise=False)
    try:
        return _to_snapshot(b)
    finally:
        b.close()


@lru_cache(maxsize=None)
def _twin(k, e):
    """Scene k after restart e at tau = K0 + K1, as the twin says; shared by the tests, nobody changes it."""
    state, wps, veh = _held()
    xy, wp, first, vehicles, fb = RC.twin(k, e, state=state[k], vehicles=veh[k], waypoints=wps[k][0], shift=K1, tau=K0 + K1)
    tr = RC.tracks()[k]
    present = np.array([scenarios.track_present(None if t is None else dict(t, first_tick=int(first[v])), K0 + K1)
                        for v, t in enumerate(tr or [])], dtype=bool)
    return {"xy": xy, "wp": wp, "first": first, "veh": vehicles, "fb": fb, "present": present}


def _expected(k, e):
    """... as _read reads it."""
    state, wps, _ = _held()
    t = _twin(k, e)
    loc = state[k][0].copy()
    loc[:, :2] = t["xy"]
    return {"loc": _bits(loc), "vel": _bits(state[k][1]), "wp": _bits(t["wp"]), "draws": wps[k][1], "ctr": [_bits(c) for c, _ in t["veh"]],
            "ring": [_bits(r) for _, r in t["veh"]], "present": t["present"], "resets": np.uint32(e + 1), "fallbacks": np.uint32(t["fb"])}


def _restart(b, path, chosen):
    mask = np.zeros(b.B, bool)
    mask[list(chosen)] = True
    if path == "host":
        b.restart(mask)
    elif path == "device":
        import torch
        b.restart_device(torch.as_tensor(mask, device="cuda"))
        torch.cuda.synchronize()
    else:
        b.end_step(auto_restart=True)
        assert np.array_equal(b.episodes()[1], mask)


@pytest.mark.parametrize("path", ["host", "device", "end_step"])
def test_three_restarts_equal_the_twin_and_leave_the_others_alone(path):
    chosen = CHOSEN[path]
    b = _build()
    try:
        if path == "end_step":                                         # a chosen scene runs out of time at every evaluation
            b.set_episodes(agent=0, max_steps=[1 if k in chosen else 0 for k in ALL])
        _to_snapshot(b)
        assert b.has_snapshot
        changed = 0
        for e in (0, 1, 2):
            before = _read(b)
            _restart(b, path, chosen)
            after = _read(b)
            for k in ALL:
                if k in chosen:
                    _same(after[k], _expected(k, e), f"{path}, restart {e}, scene {k}")
                    changed += not np.array_equal(after[k]["loc"], before[k]["loc"])
                else:
                    _same(after[k], before[k], f"{path}, restart {e}, scene {k} (not chosen)")
                    assert after[k]["resets"] == 0 and after[k]["fallbacks"] == 0
        assert changed >= 3 * (len(chosen) - 1)                        # (the scene of zero boxes stays)
        counts = b.reset_count_tensor().cpu().numpy()
        assert list(counts) == [3 if k in chosen else 0 for k in ALL]
        assert any(not _twin(k, e)["present"].all() for k in chosen for e in (0, 1, 2) if len(_twin(k, e)["present"]))
        assert sum(_twin(k, e)["fb"] for k in chosen for e in (0, 1, 2)) > 0
    finally:
        b.close()


def test_a_scene_alone_equals_the_scene_in_the_crowd():
    for k in (4, 5):                                                   # the scenes that go in passes; another index, the same seed
        b = _build((k,))
        try:
            _to_snapshot(b)
            for e in (0, 1):
                b.restart()
                _same(_read(b)[0], _expected(k, e), f"scene {k} alone, restart {e}")
        finally:
            b.close()


def test_the_tick_reads_what_was_placed():
    which = (0, 3, 4)
    tau = K0 + K1
    a = _build(which)
    state, _, held_veh = _held()
    scenes, tracks = [], []
    for k in which:
        t = _twin(k, 0)
        sc = dict(RC.scenes()[k])
        sc["loc"] = state[k][0].copy()
        sc["loc"][:, :2] = t["xy"]
        sc["vel"] = state[k][1]
        sc["waypoint"] = np.column_stack([t["wp"].astype(np.float64), RC.scenes()[k]["waypoint"][:, 2]])
        sc["dynamic_obstacles"] = [RC.scenes()[k]["dynamic_obstacles"][0], held_veh[k][1]]     # the free vehicle where the snapshot had it
        scenes.append(sc)
        tracks.append([dict(RC.tracks()[k][0], first_tick=int(t["first"][0]) - tau), None])
    f = _build(which, noise=False, scenes=scenes, tracks=tracks)
    try:
        _to_snapshot(a)
        a.restart()
        keep = ("loc", "vel", "wp", "ctr", "ring", "present")
        for ticks in (0, 3):
            if ticks:
                a.run(ticks)
                f.run(ticks)
            for got, want, k in zip(_read(a), _read(f), which):
                _same({n: got[n] for n in keep}, {n: want[n] for n in keep}, f"scene {k} after {ticks} ticks")
        assert not np.array_equal(_read(a)[1]["loc"], _expected(3, 0)["loc"])     # (the ticks moved the crowd)
    finally:
        a.close()
        f.close()


def test_a_3d_batch_keeps_z_and_vz():
    k = 3
    sc = dict(RC.scenes()[k])
    rng = np.random.default_rng(3)
    sc["loc"], sc["vel"] = sc["loc"].copy(), sc["vel"].copy()
    sc["loc"][:, 2] = scenarios._f32(rng.uniform(0.0, 1.5, RC.SIZES[k]))
    sc["vel"][:, 2] = scenarios._f32(rng.normal(0.0, 0.05, RC.SIZES[k]))
    b = _build((k,), scenes=[sc])
    try:
        assert not b.planar
        b.snapshot()
        held = (b.state()[0], b.waypoints()[0], b.dynamic_obstacles()[0])
        b.run(K1)
        b.restart()
        xy, wp, _, _, fb = RC.twin(k, 0, state=held[0], vehicles=held[2], waypoints=held[1][0], shift=K1, tau=K1)
        loc, vel = b.state()[0]
        assert np.array_equal(_bits(loc[:, :2]), _bits(xy)) and np.array_equal(_bits(b.waypoints()[0][0]), _bits(wp))
        assert np.array_equal(_bits(loc[:, 2]), _bits(held[0][0][:, 2])) and np.array_equal(_bits(vel), _bits(held[0][1]))
        assert loc[:, 2].any() and vel[:, 2].any() and b.restart_noise()[1][0] == fb
    finally:
        b.close()


def test_off_means_off():
    b = _build()
    try:
        _to_snapshot(b)
        b.set_restart_noise(None, None)
        assert b.has_snapshot and not b.has_restart_noise
        b.restart()
        state, wps, veh = _held()
        for k, ((loc, vel), (wp, d), v) in enumerate(zip(b.state(), b.waypoints(), b.dynamic_obstacles())):
            assert np.array_equal(_bits(loc), _bits(state[k][0])) and np.array_equal(_bits(vel), _bits(state[k][1])), k
            assert np.array_equal(_bits(wp), _bits(wps[k][0])) and np.array_equal(d, wps[k][1]), k
            assert all(np.array_equal(_bits(p), _bits(q)) for (_, p), (_, q) in zip(v, veh[k])), k
        with pytest.raises(SfmLibraryError, match="restart noise is off"):
            b.restart_noise()
        with pytest.raises(SfmLibraryError, match="restart noise is off"):
            b.reset_count_tensor()
    finally:
        b.close()


def _set_raw(b, args):
    sd, phx, phy, ghx, ghy, g1, g2, tries, delay = args
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = b._lib.sfm_batch_set_restart_noise(b._b, *(ptr(a) for a in (sd, phx, phy, ghx, ghy, g1, g2)), tries, ptr(delay))
    return rc, b._lib.sfm_batch_last_error(b._b).decode()


def test_refusals_leave_the_noise_that_was_set_in_force():
    which = (3, 1)
    b = _build(which)
    try:
        _to_snapshot(b)
        so = b.scene_off
        good = pack_restart_noise([1, 2], np.array([0.5, 0.5]), so, None, 0.1, 0.1, 4, np.zeros(2, np.int32), 2)
        bad_box = list(good)
        bad_box[1] = good[1].copy()
        bad_box[1][7] = -1.0
        rc, msg = _set_raw(b, bad_box)
        assert rc == SFM_ERR_INVALID and "row 7: the half-extents of a box must be finite, >= 0 and <= 1e6 metres" in msg
        for tries in (0, 33):
            rc, msg = _set_raw(b, good[:7] + (tries, good[8]))
            assert rc == SFM_ERR_INVALID and "tries must be 1 .. 32" in msg
        nan_gap = list(good)
        nan_gap[5] = np.array([0.1, np.nan], np.float32)
        rc, msg = _set_raw(b, nan_gap)
        assert rc == SFM_ERR_INVALID and "scene 1: min_gap must be finite, >= 0 and <= 1e6 metres" in msg
        rc, msg = _set_raw(b, good[:8] + (np.array([0, -1], np.int32),))
        assert rc == SFM_ERR_INVALID and "vehicle 1: track_delay must be >= 0" in msg
        b.restart()                                                    # the noise of _build is still the one in force
        for j, k in enumerate(which):
            _same(_read(b)[j], _expected(k, 0), f"scene {k} after the refusals")

        # the int32 fit of a restart adds the largest delay: refused with nothing launched, counters included
        huge = pack_restart_noise(list(np.array(RC.SEEDS)[list(which)]), np.array([0.5, 0.5]), so, None, 0.1, 0.1, 4,
                                  np.array([2**31 - 1, 0], np.int32), 2)
        assert _set_raw(b, huge)[0] == 0
        before = _read(b)
        b.set_episodes(agent=0, max_steps=0)
        for call in (lambda: b.restart(), lambda: b.restart([0]), lambda: b.restart_device(None)):
            with pytest.raises(SfmLibraryError, match="the largest delay of the restart noise, 2147483647, does not fit int32"):
                call()
        with pytest.raises(SfmLibraryError, match="does not fit int32"):
            b.end_step(auto_restart=True)
        assert not b.episodes()[0].any()                               # (no end_step has run: every refusal came before the launch)
        for got, want, k in zip(_read(b), before, which):
            _same(got, want, f"scene {k} after a refused restart")
        b.restart([1])                                                 # (a scene without tracked vehicles restarts under the same noise)
        assert list(b.restart_noise()[0]) == [0, 1]

        # track_delay without tracks: SFM_ERR_STATE, and the noise before stays
        b.set_vehicle_tracks(None)
        rc, msg = _set_raw(b, good)
        assert rc == SFM_ERR_STATE and "track_delay needs vehicle tracks" in msg
        assert list(b.restart_noise()[0]) == [0, 1]
        assert _set_raw(b, good[:8] + (None,))[0] == 0                 # (without delays it is taken)
        assert list(b.restart_noise()[0]) == [0, 0]
    finally:
        b.close()
