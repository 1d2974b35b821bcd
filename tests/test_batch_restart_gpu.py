"""GPU tests of the batch's snapshot and restart (sfm_batch_snapshot, sfm_batch_restart; SfmBatch.snapshot / restart).

The oracle is the library's own guarantee that a scene's result does not depend on the rest of the batch, so every comparison is
bitwise.  Batch A runs K0 ticks, takes a snapshot, runs K1 ticks, restarts the scenes of a mask and runs J ticks; an identically
built batch F never restarts.  A scene in the mask must equal F after K0 + J ticks, a scene outside it F after K0 + K1 + J ticks,
in everything that can be read back: state, waypoints and draw counters, vehicles, modes, clocks, births, track presence.
Four scenes of 0, 5, 70 and 300 pedestrians: an empty scene, one below a wave, one across a wave boundary and one above the
workgroup's 256 threads, so the copy loop strides.  Run on the MI355X box with  python -m pytest tests -m gpu."""
from functools import lru_cache

import numpy as np
import pytest

import test_batch_modes_gpu as M
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import SfmBatch, pack_scenes
from carla_social_force_model_amd._lib import SfmLibraryError

pytestmark = pytest.mark.gpu

SIZES = (0, 5, 70, 300)
DTS = (0.05, 0.04, 0.05, 0.03)
T0 = (4.5, 4.5, 4.5, 4.7)          # the scenes' clocks at set_modes: an IDLE row (wakes at 5 s) wakes between tick 7 and tick 16
K1, J = 9, 11
FEATURES = ("plain", "streams", "vehicles", "modes", "spawns", "tracks", "tracks3d")
MASKS = {"one": [1], "two": [0, 3], "all": None, "none": []}
SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3


def _has(feat, what):
    return {"vehicles": feat not in ("plain", "streams"), "modes": feat in ("modes", "spawns", "tracks", "tracks3d"),
            "spawns": feat == "spawns", "tracks": feat in ("tracks", "tracks3d"), "streams": feat == "streams"}[what]


@lru_cache(maxsize=None)
def _made(z3):
    """The four scenes with their mode plans, spawn schedules and tracks (built once; nothing below changes them)."""
    made = [M._scene(n, 4100 + k, 2 if n else 0, z_spread=1.5 if z3 else 0.0, borders=2) for k, n in enumerate(SIZES)]
    scenes = [m[0] for m in made]
    # one more waypoint per row: a row that arrives twice despawns, so despawns keep coming throughout the run
    plans = [scenarios.make_mode_plan(sc, 4150 + k, queue_len=1)[0] for k, sc in enumerate(scenes)]
    scheds = [scenarios.make_spawn_plan(sc, 4300 + k, dt=DTS[k], t0=T0[k], present=0.35, horizon=1.5) for k, sc in enumerate(scenes)]
    tracks = [scenarios.make_track_plan(sc, 4200 + k, 7 + K1 + J, dt=DTS[k]) if len(sc["dynamic_obstacles"]) else None
              for k, sc in enumerate(scenes)]
    return scenes, plans, scheds, tracks


def _build(feat, cfg_shift=0):
    scenes, plans, scheds, tracks = _made(feat == "tracks3d")
    b = SfmBatch([M._config(k + cfg_shift) for k in range(len(SIZES))], list(DTS))
    try:
        b.upload(scenes, device_vehicles=_has(feat, "vehicles"))
        assert b.planar == (feat != "tracks3d")
        if _has(feat, "streams"):
            b.set_waypoint_streams([11, 12, 13, 14], 30.0, 2.0)
        if _has(feat, "tracks"):
            b.set_vehicle_tracks(tracks)
        if _has(feat, "modes"):
            b.set_modes(plans, despawn_on_arrival=True, sim_time0=list(T0), arrive_thresholds=2.0, scenes=scenes)
        if _has(feat, "spawns"):
            b.set_spawns(scheds)
    except Exception:
        b.close()
        raise
    return b


def _run(b, feat, ticks):
    b.run(ticks, redraw=_has(feat, "streams"))


def _read(b, feat):
    """Everything readable, per scene: a dict name -> array (vehicles as lists of arrays)."""
    out = [{"loc": loc, "vel": vel, "wp": wp, "draws": d, "ctr": [c for c, _ in veh], "ring": [r for _, r in veh]}
           for (loc, vel), (wp, d), veh in zip(b.state(), b.waypoints(), b.dynamic_obstacles())]
    if _has(feat, "modes"):
        clocks = b.clocks()
        for k, (m, t, c) in enumerate(b.modes()):
            out[k].update(mode=m, target=t, cursor=c, clock=clocks[k:k + 1])
    if _has(feat, "spawns"):
        for k, (born, when) in enumerate(b.spawns()):
            out[k].update(born=born, birth=when)
    if _has(feat, "tracks"):
        for k, p in enumerate(b.vehicle_tracks()[1]):
            out[k].update(present=p)
    return out


def _same_array(u, v):
    u, v = np.asarray(u), np.asarray(v)
    if u.shape != v.shape or u.dtype != v.dtype:
        return False
    if u.dtype.kind == "f":                                    # NaN (an unborn row's birth time): the same places, then the rest
        nu, nv = np.isnan(u), np.isnan(v)
        return bool(np.array_equal(nu, nv) and np.array_equal(u[~nu], v[~nv]))
    return bool(np.array_equal(u, v))


def _assert_scene(got, want, what):
    assert got.keys() == want.keys(), what
    for name, u in got.items():
        v = want[name]
        if isinstance(u, list):
            assert len(u) == len(v) and all(_same_array(a, c) for a, c in zip(u, v)), f"{what}: {name}"
        else:
            assert _same_array(u, v), f"{what}: {name}"


@lru_cache(maxsize=None)
def _fresh(feat, ticks, cfg_shift=0):
    """The batch that never restarts, read out after each of ``ticks`` (ascending) ticks: {ticks: readout}.  Computed once per key
    and shared; nobody changes it."""
    f = _build(feat, cfg_shift)
    try:
        out, done = {}, 0
        for t in ticks:
            _run(f, feat, t - done)
            done = t
            out[t] = _read(f, feat)
        return out
    finally:
        f.close()


def _chosen(mask):
    return set(range(len(SIZES))) if mask is None else set(mask)


def _something_happens(feat, first, mid, last):
    """On F itself, over its readouts (K0, K0 + J, K0 + K1 + J): the feature's state changed, so a restart that copied nothing
    could not pass.  Presence is looked at in all three: a vehicle that enters and leaves inside the run is absent at both ends."""
    rows = lambda r, name: np.concatenate([s[name].reshape(-1) for s in r])
    assert not np.array_equal(rows(first, "loc"), rows(last, "loc"))
    if _has(feat, "streams"):
        assert rows(last, "draws").sum() > rows(first, "draws").sum()
    if _has(feat, "vehicles"):
        assert any(not _same_array(a, c) for s, t in zip(first, last) for a, c in zip(s["ctr"], t["ctr"]))
    if _has(feat, "modes"):
        assert (rows(first, "mode") != rows(last, "mode")).any() and (rows(first, "cursor") != rows(last, "cursor")).any()
        assert (rows(last, "mode") == M.GONE).sum() > (rows(first, "mode") == M.GONE).sum()      # a despawn inside the run
        woke = (rows(first, "mode") == 0) & (rows(last, "mode") != 0) & (rows(last, "mode") != M.GONE)
        assert woke.any()                                                                          # an IDLE timer that expired
    if _has(feat, "spawns"):
        assert rows(last, "born").sum() > rows(first, "born").sum()
    if _has(feat, "tracks"):
        assert (rows(first, "present") != rows(mid, "present")).any() or (rows(mid, "present") != rows(last, "present")).any()


@pytest.mark.parametrize("mask", list(MASKS), ids=list(MASKS))
@pytest.mark.parametrize("k0", [0, 7])
@pytest.mark.parametrize("feat", FEATURES)
def test_restarted_scenes_start_over_and_the_others_go_on(feat, k0, mask):
    chosen = MASKS[mask]
    fresh = _fresh(feat, (k0, k0 + J, k0 + K1 + J))
    _something_happens(feat, fresh[k0], fresh[k0 + J], fresh[k0 + K1 + J])
    if _has(feat, "spawns") and k0:                                    # births before the snapshot and after it
        born = lambda r: sum(int(s["born"].sum()) for s in r)
        assert born(_fresh(feat, (0, J, K1 + J))[0]) < born(fresh[k0]) < born(fresh[k0 + K1 + J])
    a = _build(feat)
    try:
        _run(a, feat, k0)
        a.snapshot()
        assert a.has_snapshot
        _run(a, feat, K1)
        a.restart(chosen)
        _run(a, feat, J)
        got = _read(a, feat)
        for k in range(len(SIZES)):
            back = k in _chosen(chosen)
            _assert_scene(got[k], fresh[k0 + J if back else k0 + K1 + J][k],
                          f"{feat}, K0 = {k0}, mask {mask}: scene {k} ({'restarted' if back else 'left alone'})")
        if _has(feat, "tracks"):                                       # tau stays the batch's one counter
            assert a.vehicle_tracks()[0] == k0 + K1 + J
    finally:
        a.close()


@pytest.mark.parametrize("feat", ["tracks", "spawns"])
def test_restart_twice(feat):
    """restart {2}, 5 ticks, restart {2} again, J ticks: scene 2 is F after K0 + J ticks, tracks included (a shift of the first
    ticks applied on top of the earlier one would leave its vehicles 5 keyframes off); the others are F after every tick run."""
    k0 = 7
    fresh = _fresh(feat, (k0 + J, k0 + K1 + 5 + J))
    a = _build(feat)
    try:
        _run(a, feat, k0)
        a.snapshot()
        _run(a, feat, K1)
        a.restart([2])
        _run(a, feat, 5)
        a.restart(np.array([False, False, True, False]))
        _run(a, feat, J)
        got = _read(a, feat)
        for k in range(len(SIZES)):
            _assert_scene(got[k], fresh[k0 + J if k == 2 else k0 + K1 + 5 + J][k], f"{feat}: scene {k}")
    finally:
        a.close()


def test_a_second_snapshot_replaces_the_first():
    feat = "tracks"
    fresh = _fresh(feat, (3 + J, 3 + K1 + J))
    a = _build(feat)
    try:
        a.snapshot()
        _run(a, feat, 3)
        a.snapshot()
        _run(a, feat, K1)
        a.restart([1, 2])
        _run(a, feat, J)
        got = _read(a, feat)
        for k in range(len(SIZES)):
            _assert_scene(got[k], fresh[3 + J if k in (1, 2) else 3 + K1 + J][k], f"scene {k}")
    finally:
        a.close()


@pytest.mark.parametrize("feat", ["modes", "tracks3d"])
def test_recorded_run_after_a_restart_starts_at_the_snapshot(feat):
    """run_recorded(J) straight after a restart: frame 0 of a restarted scene is bitwise its state at the snapshot, frame 0 of
    the others their state before the restart; the run ends where F ends."""
    k0 = 7
    fresh = _fresh(feat, (k0, k0 + J, k0 + K1 + J))
    a = _build(feat)
    try:
        _run(a, feat, k0)
        a.snapshot()
        at_snapshot = a.state()
        _run(a, feat, K1)
        before_restart = a.state()
        a.restart([1, 3])
        frames, idx, zframes = a.run_recorded(J)
        assert list(idx) == list(range(J))
        for k in range(len(SIZES)):
            loc, vel = (at_snapshot if k in (1, 3) else before_restart)[k]
            f0 = frames[k][0].astype(np.float64)
            assert np.array_equal(f0[:, :2], loc[:, :2]) and np.array_equal(f0[:, 2:], vel[:, :2]), f"scene {k}: frame 0"
            if zframes is not None:
                z0 = zframes[k][0].astype(np.float64)
                assert np.array_equal(z0[:, 0], loc[:, 2]) and np.array_equal(z0[:, 1], vel[:, 2]), f"scene {k}: z frame 0"
            assert _same_array(at_snapshot[k][0], fresh[k0][k]["loc"])
        got = _read(a, feat)
        for k in range(len(SIZES)):
            _assert_scene(got[k], fresh[k0 + J if k in (1, 3) else k0 + K1 + J][k], f"scene {k} after the recorded run")
    finally:
        a.close()


def test_sweep_restarts_under_the_parameters_of_the_moment():
    """snapshot(), run(9), set_params(other configs), restart(), run(J) equals a fresh batch built with the other configs after J
    ticks; set_params and set_waypoint_streams keep the snapshot."""
    feat = "modes"
    fresh = _fresh(feat, (J,), 1)
    assert not _same_array(fresh[J][3]["vel"], _fresh(feat, (0, J, K1 + J))[J][3]["vel"])       # the other configs matter
    a = _build(feat)
    try:
        a.snapshot()
        _run(a, feat, 9)
        a.set_params([M._config(k + 1) for k in range(len(SIZES))], list(DTS))
        a.set_waypoint_streams(5, 30.0, 2.0)
        assert a.has_snapshot
        a.restart()
        _run(a, feat, J)
        got = _read(a, feat)
        for k in range(len(SIZES)):
            _assert_scene(got[k], fresh[J][k], f"scene {k}")
    finally:
        a.close()


def test_refusals_leave_the_batch_usable():
    """No snapshot, a mask value of 2, a first tick that would leave int32: an SfmLibraryError (or the C status) with nothing
    launched; the batch runs on and matches F."""
    feat = "tracks"
    fresh = _fresh(feat, (3 + J, 3 + K1 + J))
    scenes = _made(False)[0]
    a = SfmBatch([M._config(k) for k in range(len(SIZES))], list(DTS))
    try:
        with pytest.raises(SfmLibraryError, match="sfm_batch_upload_state has not been called"):
            a.snapshot()
        assert not a.has_snapshot
        with pytest.raises(SfmLibraryError, match="no snapshot"):
            a.restart()
    finally:
        a.close()
    a = _build(feat)
    L = a._lib
    try:
        _run(a, feat, 3)
        with pytest.raises(SfmLibraryError, match="no snapshot"):
            a.restart()
        with pytest.raises(SfmLibraryError, match="no snapshot"):
            a.restart([1])
        a.snapshot()
        _run(a, feat, K1)
        bad = np.array([0, 1, 2, 0], dtype=np.uint8)
        assert L.sfm_batch_restart(a._b, _lib.u8ptr(bad)) == SFM_ERR_INVALID
        assert "mask must hold 0 or 1 (scene 2)" in L.sfm_batch_last_error(a._b).decode()
        with pytest.raises(ValueError):
            a.restart([4])
        assert a.has_snapshot
        a.restart([1, 2])                                              # the snapshot is still there
        _run(a, feat, J)
        got = _read(a, feat)
        for k in range(len(SIZES)):
            _assert_scene(got[k], fresh[3 + J if k in (1, 2) else 3 + K1 + J][k], f"scene {k}")
        # a first tick at the end of int32: one tick after the snapshot it cannot move any further
        tracks = [None if t is None else [dict(t[0], first_tick=2**31 - 1), t[1]] for t in _made(False)[3]]
        a.set_vehicle_tracks(tracks)
        assert not a.has_snapshot
        a.snapshot()
        _run(a, feat, 1)
        before = _read(a, feat)
        with pytest.raises(SfmLibraryError, match="set the tracks again"):
            a.restart([3])
        with pytest.raises(SfmLibraryError, match="set the tracks again"):
            a.restart()
        a.restart([0])                                                 # the empty scene has no vehicle: nothing to move
        for k, (u, v) in enumerate(zip(_read(a, feat), before)):
            if k:
                _assert_scene(u, v, f"after the refused restarts: scene {k}")
        _run(a, feat, 1)
        assert a.vehicle_tracks()[0] == 2
    finally:
        a.close()


def test_calls_that_drop_the_snapshot():
    """Each call that changes which arrays exist drops the snapshot, in its "off" form too; restart() is then refused, touches
    nothing, and the batch runs on.  A refused call drops nothing."""
    feat = "tracks"
    scenes, plans, scheds, tracks = _made(False)
    a = _build(feat)
    L = a._lib
    modes = lambda: a.set_modes(plans, despawn_on_arrival=True, sim_time0=list(T0), arrive_thresholds=2.0, scenes=scenes)
    dy = pack_scenes(scenes)["dynamic"]
    rings = lambda: a._check_drops(L.sfm_batch_set_dynamic_obstacles(a._b, *(_lib.iptr(x) for x in dy[:2]),
                                                                     *(_lib.fptr(x) for x in dy[2:])), "sfm_batch_set_dynamic_obstacles")
    calls = [("set_vehicle_tracks(None)", lambda: a.set_vehicle_tracks(None)),
             ("set_vehicle_tracks", lambda: a.set_vehicle_tracks(tracks)),
             ("set_spawns(None)", lambda: a.set_spawns(None)),
             ("set_modes(None)", lambda: a.set_modes(None)),
             ("set_modes", modes),
             ("set_spawns", lambda: a.set_spawns(scheds)),
             ("set_dynamic_boxes", lambda: a.set_dynamic_boxes(scenes)),
             ("sfm_batch_set_dynamic_obstacles", rings),
             ("upload", lambda: a.upload(scenes, device_vehicles=True))]
    readable = lambda: [(loc, vel, wp, d, [c for c, _ in veh], [r for _, r in veh])
                        for (loc, vel), (wp, d), veh in zip(a.state(), a.waypoints(), a.dynamic_obstacles())]
    try:
        a.run(3)
        for name, call in calls:
            a.snapshot()
            assert a.has_snapshot, name
            a.run(1)
            call()
            assert not a.has_snapshot, name
            before = readable()
            with pytest.raises(SfmLibraryError, match="no snapshot"):
                a.restart()
            assert L.sfm_batch_restart(a._b, None) == SFM_ERR_STATE, name
            for x, y in zip(before, readable()):
                for u, v in zip(x, y):
                    assert all(_same_array(p, q) for p, q in zip(u, v)) if isinstance(u, list) else _same_array(u, v), name
            a.run(1)
            if name == "set_spawns":                                   # a second schedule is refused: that drops nothing
                a.snapshot()
                with pytest.raises(SfmLibraryError, match="already been set"):
                    a.set_spawns(scheds)
                with pytest.raises(SfmLibraryError, match="device-side vehicles|NULL|non-decreasing|trk_off"):
                    a._check_drops(L.sfm_batch_set_vehicle_tracks(a._b, _lib.iptr(np.ones(1, np.int32)), *([None] * 7)),
                                   "sfm_batch_set_vehicle_tracks")
                assert a.has_snapshot
                a.restart()
                a.run(1)
    finally:
        a.close()
