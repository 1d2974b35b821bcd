"""GPU tests of range scans on a batch (sfm_batch_set_scan, sfm_batch_scan, sfm_batch_download_scan, SFM_BATCH_PTR_SCAN;
SfmBatch.set_scan / scan / scans / scan_tensor): bitwise against the host twin ``scan.scan_scene`` in BOTH frames, designed ties,
independence of the rest of the batch, that scanning changes nothing, moving geometry and ghosts, restarts, the device view, and
every refusal.  No tolerance appears anywhere."""
import ctypes as C
import importlib.util
import os
from functools import lru_cache

import numpy as np
import pytest

import test_batch_gpu as G
import test_batch_modes_gpu as M
import test_batch_tracks_gpu as T
import test_batch_vehicles_gpu as V
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd._lib import SfmLibraryError
from carla_social_force_model_amd.batch import PTR_SCAN, SfmBatch
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.scan import default_angles, range_census, ray_directions, scan_scene

pytestmark = pytest.mark.gpu

SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3
SIZES = (0, 1, 2, 3, 17, 64, 65, 129, 300, 1024, 40, 90)               # the last two carry 3 vehicles each
RS = (1, 8, 33, 64)
RMAX = (2.5, 4.0, 6.0)                                                 # per scene, in turn
PED = (0.3, 0.45, 0.2)
POINT = (0.1, 0.25, 0.1)
AXES = (np.float32([1, 0, -1, 0]), np.float32([0, 1, 0, -1]))


def _settings(B):
    return [RMAX[b % 3] for b in range(B)], [PED[b % 3] for b in range(B)], [POINT[b % 3] for b in range(B)]


@lru_cache(maxsize=None)
def _scenes(z3=False):
    """The mixed batch.  Row 1 of the 17-row scene stands inside row 0's disc.  The 3-D form has the planar form's x, y, vx, vy,
    with a z and a vz of its own per row."""
    scenes = [G._scene(n, 5000 + q, dynamic=3 if q >= 10 else 0) for q, n in enumerate(SIZES)]
    scenes[4]["loc"] = np.array(scenes[4]["loc"])
    scenes[4]["loc"][1, :2] = scenes[4]["loc"][0, :2] + np.float32(0.125)
    if z3:
        rng = np.random.default_rng(5)
        for sc in scenes:
            n = len(sc["loc"])
            sc["loc"] = np.column_stack([sc["loc"][:, :2], rng.uniform(0.0, 1.5, n)])
            sc["vel"] = np.column_stack([sc["vel"][:, :2], rng.uniform(-0.2, 0.2, n)])
    return scenes


@lru_cache(maxsize=None)
def _masks():
    """Every row of every scene, but about 40 rows of the 1 024-row scene."""
    masks = [np.ones(n, bool) for n in SIZES]
    masks[9] = np.zeros(1024, bool)
    masks[9][3::26] = True
    return masks


@lru_cache(maxsize=None)
def _twin(R, frame=0):
    rm, pr, qr = _settings(len(SIZES))
    return [scan_scene(sc, default_angles(R), rm[s], pr[s], qr[s], frame=frame, mask=_masks()[s]) for s, sc in enumerate(_scenes())]


def _batch(scenes, planar=None, device_vehicles=False):
    b = SfmBatch(default_sfm_config(), 0.05, B=len(scenes))
    b.upload(scenes, planar=planar, device_vehicles=device_vehicles)
    return b


def _scanned(scenes, rmax, ped, point, planar=None, **kw):
    b = _batch(scenes, planar)
    try:
        b.set_scan(rmax, ped, point, **kw)
        return b.scans()
    finally:
        b.close()


@lru_cache(maxsize=None)
def _device(R, frame, z3):
    return _scanned(_scenes(z3), *_settings(len(SIZES)), R=R, frame=frame, mask=list(_masks()))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, what
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} floats differ, first (row, float) {bad[0]}: {got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}"


# ---- 1. classes, from the twin alone ---------------------------------------------------------------------------------------------

def test_the_batch_holds_every_class():
    R = 64
    rec = np.concatenate(_twin(R))
    rm = np.concatenate([np.full(n, np.float32(r), np.float32) for n, r in zip(SIZES, _settings(len(SIZES))[0])])
    scanned = np.concatenate(_masks())
    rng, kind = rec[:, :R], rec[:, R:]
    assert ((kind == 0) & (rng == rm[:, None]))[scanned].any()                          # a ray with no hit
    for k in (1, 2, 3, 4):
        assert (kind == k).any(), k                                                   # a hit of each kind
    assert ((rng == 0) & (kind > 0)).any()                                             # inside a disc
    assert (np.array([len(set(r) - {0.0}) for r in kind]) >= 2).any()                   # a row with mixed kinds
    masked = ~scanned
    assert masked.any() and not rec[masked].any() and (scanned[1:] & masked[:-1]).any()
    census = sum(range_census(sc, default_angles(R), r, p, q, mask=m)
                 for sc, r, p, q, m in zip(_scenes(), *_settings(len(SIZES)), _masks()))
    for k in (1, 2, 3, 4):
        assert census[k, 0] > 0 and census[k, 1] > 0, f"kind {k}: {census[k]} candidates just inside / just outside the range limit"
    for frame in (0, 1):                                                               # frame 1 is another record
        for R in RS:
            assert sum(len(t) for t in _twin(R, frame)) == sum(SIZES)
    assert any((a != b).any() for a, b in zip(_twin(8, 0), _twin(8, 1)) if len(a))


# ---- 2. bitwise against the twin ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("R", RS)
def test_device_is_bitwise_the_twin(R, frame, z3):
    got, want = _device(R, frame, z3), _twin(R, frame)
    assert len(got) == len(SIZES)
    for s, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"scene {s} (N = {SIZES[s]}), R = {R}, frame {frame}")


# ---- 3. designed ties -----------------------------------------------------------------------------------------------------------

def _lattice():
    xy = np.array([[c, r] for r in range(5) for c in range(5)], dtype=np.float64)
    sc = G._scene(25, 77, geo=False)
    sc["loc"] = np.column_stack([xy, np.zeros(25)])
    return sc


def _grazing(with_hit):
    """Row 0 looks along +x past discs of radius 0.5 whose centres sit 0.5 off the ray, give or take one ulp: q > 0 (only
    ``with_hit``), q = 0 and q < 0.  The same three offsets, as border points, stand beside the +y ray."""
    lo, hi = np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))
    peds = [[0, 0]] + ([[3, lo]] if with_hit else []) + [[5, 0.5], [7, hi]]
    sc = G._scene(len(peds), 78, geo=False)
    sc["loc"] = np.column_stack([np.float64(peds), np.zeros(len(peds))])
    sc["borders"] = [np.float64([[0.5, 5.0], [hi, 7.0], [lo, 9.0]])]
    sc["border_centers"] = np.float64([[0.5, 7.0]])
    sc["border_lengths"] = np.float64([4.0])
    return sc


def test_designed_ties():
    lat = _lattice()
    pair = G._scene(17, 5100)
    pair["loc"] = np.array(pair["loc"])
    pair["loc"][6] = pair["loc"][5]
    graze, miss = _grazing(True), _grazing(False)
    scenes, rm, pr, qr = [lat, pair, graze, miss], [10.0, 4.0, 20.0, 20.0], [0.25, 0.3, 0.5, 0.5], [0.1, 0.1, 0.5, 0.5]
    for frame in (0, 1):
        got = _scanned(scenes, rm, pr, qr, directions=AXES, frame=frame)
        for s, sc in enumerate(scenes):
            _same(got[s], scan_scene(sc, None, rm[s], pr[s], qr[s], frame=frame, directions=AXES), f"scene {s}, frame {frame}")
    got = _scanned(scenes, rm, pr, qr, directions=AXES)
    assert np.array_equal(got[0][12], np.float32([0.75, 0.75, 0.75, 0.75, 1, 1, 1, 1]))   # the lattice's centre: four equal ranges
    assert np.array_equal(got[0][0, :4], np.float32([0.75, 0.75, 10, 10]))
    assert not got[1][5, :4].any() and (got[1][5, 4:] == 1).all()                      # the coincident pair: inside each other
    assert got[2][0, 4] == 1 and 2.9 < got[2][0, 0] < 3.0                              # q > 0 by one ulp: a hit, just
    assert got[2][0, 5] == 2 and 8.9 < got[2][0, 1] < 9.0                              # ... the third border point, not the first two
    assert got[3][0, 4] == 0 and got[3][0, 0] == 20.0                                  # q = 0 and q < 0: misses
    got8 = _scanned([lat], 10.0, 0.25, 0.1, R=8)
    _same(got8[0], scan_scene(lat, default_angles(8), 10.0, 0.25, 0.1), "lattice, 8 rays")


# ---- 4. independence ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
def test_a_scene_does_not_depend_on_the_rest_of_the_batch(z3):
    scenes, (rm, pr, qr), R = _scenes(z3), _settings(len(SIZES)), 33
    mixed = _device(R, 1, z3)
    for s in (11, 8):                                                   # 90 rows with vehicles; 300 rows
        alone = _scanned([scenes[s]], [rm[s]], [pr[s]], [qr[s]], planar=not z3, R=R, frame=1)
        order = [4, s, 0, 3]
        moved = _scanned([scenes[q] for q in order], [2.0, rm[s], 3.0, 3.0], [0.1, pr[s], 0.3, 0.3], [0.3, qr[s], 0.0, 0.2],
                         planar=not z3, R=R, frame=1)
        assert np.array_equal(_bits(alone[0]), _bits(mixed[s])), f"scene {s} alone"
        assert np.array_equal(_bits(moved[1]), _bits(mixed[s])), f"scene {s} at position 1 of another batch"


def test_a_3d_batch_gives_the_planar_record():
    for R in (1, 64):
        for frame in (0, 1):
            for s, (a, b) in enumerate(zip(_device(R, frame, False), _device(R, frame, True))):
                assert np.array_equal(_bits(a), _bits(b)), f"R = {R}, frame {frame}, scene {s}"


# ---- 5. scanning changes nothing ------------------------------------------------------------------------------------------------

def _modes_batch():
    made = [M._scene(n, 5300 + q, 2 if n else 1) for q, n in enumerate((64, 0, 130, 17))]
    scenes, plans = [m[0] for m in made], [m[1] for m in made]
    return M._batch(scenes, plans, [M._config(q) for q in range(4)], [0.05, 0.04, 0.03, 0.05])


def _all(b):
    rows, clocks = M._everything(b)
    return rows, clocks, [[np.concatenate([c.reshape(-1), r.reshape(-1)]) for c, r in veh] for veh in b.dynamic_obstacles()]


def _assert_all(x, y, what):
    M._assert_same(x[:2], y[:2], what)
    for k, (u, v) in enumerate(zip(x[2], y[2])):
        assert len(u) == len(v) and all(np.array_equal(p, q) for p, q in zip(u, v)), f"{what}: vehicles of scene {k}"


def test_scanning_changes_nothing():
    a, b = _modes_batch(), _modes_batch()
    try:
        a.set_scan(5.0, 0.3, R=16, frame=1)
        a.run(3)
        before = _all(a)
        a.scan()
        first = a.scans()
        _assert_all(_all(a), before, "state, waypoints, modes, clocks, vehicles around scan()")
        a.run(5)
        a.scan()
        a.run(5)
        b.run(13)
        _assert_all(_all(a), _all(b), "run(3), scan, run(5), scan, run(5) against run(13)")
        assert any((x != y).any() for x, y in zip(first, a.scans()) if len(x))
    finally:
        a.close()
        b.close()


# ---- 6. moving geometry and ghosts ----------------------------------------------------------------------------------------------

def test_ghosts_are_zero_and_unseen():
    """Modes, despawn on arrival and a spawn schedule, run until a row has despawned while another is still unborn: their records
    are zero and nobody's ray ends on them (the twin, fed with the downloaded state, says what every ray ends on)."""
    sizes = (64, 17, 130)
    made = [M._scene(n, 5400 + q, 2) for q, n in enumerate(sizes)]
    scenes, plans = [m[0] for m in made], [m[1] for m in made]
    scheds = [scenarios.make_spawn_plan(sc, 9 + q, horizon=6.0) for q, sc in enumerate(scenes)]
    for sd in scheds:
        sd["spawn_time"][-1] = np.inf                                   # never born
        sd["chain"][-1] = 0
    b = M._batch(scenes, plans, [M._config(q) for q in range(3)], [0.05, 0.04, 0.05])
    try:
        b.set_spawns(scheds)
        b.set_scan(4.0, 0.3, 0.1, R=33, frame=1)
        found = False
        for _ in range(100):
            b.run(10)
            modes = [m for m, _, _ in b.modes()]
            if all((m == M.GONE).any() for m in modes) and all((m == 254).any() for m in modes):
                found = True
                break
        assert found, "no tick with a despawned and an unborn row in every scene"
        got, veh = b.scans(), b.dynamic_obstacles()
        for s, ((loc, vel), (wp, _)) in enumerate(zip(b.state(), b.waypoints())):
            ghost = (modes[s] == M.GONE) | (modes[s] == 254)
            assert ghost.any() and not ghost.all()
            assert not got[s][ghost].any(), f"scene {s}: a ghost's record"
            assert got[s][~ghost].any(axis=1).all()
            _same(got[s], scan_scene(scenes[s], default_angles(33), 4.0, 0.3, 0.1, frame=1, state=(loc, vel), vehicles=veh[s], waypoints=wp),
                  f"scene {s}")
    finally:
        b.close()


def test_vehicles_as_the_next_tick_reads_them():
    """Device-side vehicles after run(7): the records equal the twin fed with the state and dynamic_obstacles().  Tracked vehicles
    outside their keyframes are absent: no ray ends on a vehicle."""
    scenes = [V._scene(n, 5500 + q, m, slow=False) for q, (n, m) in enumerate(((64, 3), (30, 2), (0, 1), (130, 5)))]
    b = V._batch(scenes, [V._config(q, V.ALL) for q in range(4)], [0.05, 0.04, 0.05, 0.03])
    ang = default_angles(64)
    try:
        b.set_scan(30.0, 0.3, 0.1, R=64)
        b.run(7)
        got, veh = b.scans(), b.dynamic_obstacles()
        for s, (loc, vel) in enumerate(b.state()):
            _same(got[s], scan_scene(scenes[s], ang, 30.0, 0.3, 0.1, state=(loc, vel), vehicles=veh[s]), f"scene {s} after run(7)")
        assert any((o[:, 64:] == 4).any() for o in got)
        # tracks: scene 0's vehicles leave after 3, 5 and 4 keyframes; every other scene's run free
        rng = np.random.default_rng(3)
        tracks = [[T._track(rng, 3, 0, T._mid(scenes[0])), T._track(rng, 5, 0, T._mid(scenes[0])), T._track(rng, 4, 0, T._mid(scenes[0]))],
                  None, None, None]
        b.set_vehicle_tracks(tracks)
        for tau, gone in ((0, False), (4, False), (6, True)):
            while b.vehicle_tracks()[0] < tau:
                b.run(1)
            got, veh = b.scans(), b.dynamic_obstacles()
            loc, vel = b.state()[0]
            _same(got[0], scan_scene(scenes[0], ang, 30.0, 0.3, 0.1, state=(loc, vel), vehicles=veh[0]), f"tracked scene at tau = {tau}")
            assert (got[0][:, 64:] == 4).any() != gone
            assert (got[3][:, 64:] == 4).any()                          # the free vehicles of another scene are still seen
    finally:
        b.close()


# ---- 7. lifetime ----------------------------------------------------------------------------------------------------------------

def test_restarted_scenes_read_what_they_read_at_the_snapshot():
    scenes = [G._scene(n, 5600 + q) for q, n in enumerate((30, 65, 0, 130, 17))]
    rm = (2.5, 4.0, 6.0, 4.0, 6.0)
    b = _batch(scenes)
    try:
        b.set_scan(rm, 0.3, R=8, frame=1)
        b.run(3)
        b.snapshot()
        at_snapshot = b.scans()
        b.run(20)
        b.restart([1, 3])
        assert b.has_snapshot
        got = b.scans()
        for s, ((loc, vel), (wp, _)) in enumerate(zip(b.state(), b.waypoints())):
            if s in (1, 3):
                assert np.array_equal(_bits(got[s]), _bits(at_snapshot[s])), f"restarted scene {s}"
            else:
                _same(got[s], scan_scene(scenes[s], default_angles(8), rm[s], 0.3, 0.1, frame=1, state=(loc, vel), waypoints=wp), f"scene {s} went on")
                assert not len(got[s]) or (got[s] != at_snapshot[s]).any()
        b.upload(scenes)                                                # drops the scans
        assert b.scan_rays is None
        with pytest.raises(SfmLibraryError, match="scans are off"):
            b.scan()
    finally:
        b.close()


# ---- 8. device view -------------------------------------------------------------------------------------------------------------

def test_device_view():
    import torch
    scenes = [G._scene(n, 5700 + q) for q, n in enumerate((17, 0, 65))]
    b = _batch(scenes)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        b.set_scan(4.0, 0.3, R=8)
        ptr, nbytes = b.device_ptr(PTR_SCAN)
        t = b.scan_tensor()
        assert t.shape == (82, 16) and t.dtype == torch.float32 and t.data_ptr() == ptr and nbytes == 82 * 16 * 4
        assert not t.any().item()                                       # zero-filled before the first scan
        b.run(2)
        b.scan()
        seen = t.cpu().numpy()                                          # (torch's stream: ordered behind the launch)
        assert np.array_equal(seen, np.concatenate(b.scans()))
        assert np.array_equal(seen, np.concatenate([scan_scene(sc, default_angles(8), 4.0, 0.3, 0.1, state=st) for sc, st in zip(scenes, b.state())]))
        b.set_scan(4.0, 0.3, R=33)                                      # a new buffer: the view is taken again
        assert b.scan_tensor().shape == (82, 66)
    finally:
        b.close()
    e = _batch([G._scene(0, 1)])                                        # without rows: no buffer, an empty view
    try:
        e.set_scan(4.0, 0.3, R=8)
        e.scan()
        assert e._lib.sfm_batch_device_ptr(e._b, PTR_SCAN, None) is None
        assert e.scan_tensor().shape == (0, 16) and e.scans()[0].shape == (0, 16)
    finally:
        e.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_batch_usable():
    scenes = [G._scene(n, 5800 + q) for q, n in enumerate((17, 65))]
    L = _lib.load()
    err = lambda x: L.sfm_batch_last_error(x._b).decode()
    fp, up = _lib.fptr, _lib.u8ptr
    dx, dy = ray_directions(default_angles(8))
    rm, pr, qr = np.float32([3.0, 5.0]), np.float32([0.3, 0.4]), np.float32([0.1, 0.2])
    mask = np.zeros(82, np.uint8)
    mask[::3] = 1

    def set_scan(R=8, dx=dx, dy=dy, rm=rm, pr=pr, qr=qr, mask=mask, frame=0):
        return L.sfm_batch_set_scan(b._b, R, fp(dx), fp(dy), fp(rm), fp(pr), fp(qr), up(mask), frame)

    b = SfmBatch(default_sfm_config(), 0.05, B=2)
    try:
        assert set_scan() == SFM_ERR_STATE and "sfm_batch_upload_state" in err(b)
        with pytest.raises(SfmLibraryError, match="upload"):
            b.set_scan(3.0, 0.3, R=8)
        b.upload(scenes)

        def off(what):
            assert L.sfm_batch_scan(b._b) == SFM_ERR_STATE and "scans are off" in err(b), what
            out = np.zeros(82 * 16, np.float32)
            assert L.sfm_batch_download_scan(b._b, fp(out)) == SFM_ERR_STATE and "scans are off" in err(b), what
            nbytes = C.c_int64(7)
            assert L.sfm_batch_device_ptr(b._b, PTR_SCAN, C.byref(nbytes)) is None and nbytes.value == 0 and "scans are off" in err(b), what
            for call in (b.scan, b.scans, b.scan_tensor):
                with pytest.raises(SfmLibraryError, match="scans are off"):
                    call()

        def usable(what):
            got = b.scans()
            so = b.scene_off
            for s, (loc, vel) in enumerate(b.state()):
                want = scan_scene(scenes[s], default_angles(8), rm[s], pr[s], qr[s], state=(loc, vel), mask=mask[so[s]:so[s + 1]])
                _same(got[s], want, f"{what}: scene {s}")
            b.run(2)

        refused = [dict(R=0), dict(R=65), dict(R=-1), dict(frame=2), dict(frame=-1), dict(dx=None), dict(dy=None), dict(pr=None),
                   dict(qr=None), dict(dx=np.float32([np.nan] + [0] * 7)), dict(dy=np.float32([0] * 7 + [np.inf]))]
        refused += [dict(rm=np.float32([3.0, bad])) for bad in (np.nan, 0.0, -1.0, np.inf, 2.0e6)]
        refused += [dict(pr=np.float32([0.3, bad])) for bad in (np.nan, -0.1, np.inf, 2.0e6)]
        refused += [dict(qr=np.float32([bad, 0.1])) for bad in (np.nan, -0.1, np.inf, 2.0e6)]
        off("before set_scan")
        for kw in refused:
            assert set_scan(**kw) == SFM_ERR_INVALID, kw
        assert "scene 0: point_radius" in err(b)
        off("after refused calls on a batch without scans")
        for bad in (dict(R=0), dict(R=65), dict(angles=[np.nan]), dict(R=8, angles=[0.0]), dict(), dict(R=8, frame=2),
                    dict(R=8, mask=np.ones(5, bool)), dict(R=8, directions=AXES)):
            with pytest.raises(ValueError):
                b.set_scan(3.0, 0.3, **bad)
        for bad in ((np.nan, 0.3, 0.1), (3.0, -0.3, 0.1), (3.0, 0.3, np.inf), ([3.0, 3.0, 3.0], 0.3, 0.1)):
            with pytest.raises(ValueError):
                b.set_scan(*bad, R=8)
        with pytest.raises(ValueError, match="ped_radius"):
            b.set_scan(3.0, R=8)
        b.run(2)
        good = lambda: b.set_scan(rm, pr, qr, R=8, mask=mask != 0)
        good()
        usable("first settings")
        for kw in refused:
            assert set_scan(**kw) == SFM_ERR_INVALID, kw
            usable(f"after the refused {sorted(kw)}")                    # nothing changed: 8 rays, frame 0, the mask, the settings
        b.snapshot()
        good()                                                           # keeps the snapshot
        assert b.has_snapshot
        b.restart()
        b.set_scan(None)
        off("after set_scan(None)")
        b.run(1)
        good()
        usable("set again after off")
        b.upload(scenes)                                                 # drops the settings
        off("after upload")
        good()
        usable("set again after upload")
    finally:
        b.close()


# ---- the example ----------------------------------------------------------------------------------------------------------------

def test_lidar_loop_example_runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("batch_lidar_loop", os.path.join(root, "examples", "batch_lidar_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    episodes, arrivals = ex.run(B=8, steps=12, repeat=2, max_age=5, quiet=True)
    assert episodes >= 8 and 0 <= arrivals <= episodes                  # everyone runs out of time at least once
