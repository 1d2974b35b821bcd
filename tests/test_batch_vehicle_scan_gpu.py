"""GPU tests of the vehicles' range scan (sfm_batch_set_vehicle_scan, sfm_batch_scan_vehicles, sfm_batch_download_vehicle_scan;
SfmBatch.set_vehicle_scan / scan_vehicles / vehicle_scans / vehicle_scan_tensor): the record against the host twin
scan.scan_vehicles_scene BIT FOR BIT -- there is no tolerance anywhere -- on the batch of tests/_vehicle_scan_cases.py, whose classes
test_batch_vehicle_scan_host.py asserts.  Run on the MI355X box with  python -m pytest tests -m gpu."""
import numpy as np
import pytest

import _vehicle_scan_cases as VC
import test_batch_vehicles_gpu as V
from carla_social_force_model_amd import _lib, scan as S
from carla_social_force_model_amd.batch import PTR_VEHICLE_SCAN, SfmBatch, SfmLibraryError, pack_scenes

pytestmark = pytest.mark.gpu

ZERO, CASES = VC.ZERO, VC.CASES


def _batch(R, frame, mount, mask, planar=None, finite=False, scan=True):
    scenes, cfgs, tracks = VC.made(finite)
    b = V._batch(scenes, cfgs, VC.DTS, planar)
    try:
        b.set_vehicle_tracks(tracks)
        if scan:
            b.set_vehicle_scan(VC.RMAX, VC.PED, VC.POINT, angles=VC.fan(R), mask=VC.mask_arg(mask), frame=frame, mount=mount)
    except Exception:
        b.close()
        raise
    return b, scenes, tracks


def _same(got, want, what):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.float32, f"{what}: scene {s} shape {g.shape} for {w.shape}"
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), \
            f"{what}: scene {s}, vehicles {np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).any(axis=1))}"


@pytest.mark.parametrize("R,frame,mount,mask,planar", CASES, ids=[f"R{c[0]}-f{c[1]}-{'m' if c[2] != ZERO else 'c'}-{c[3]}-{'3d' if c[4] is False else 'xy'}"
                                                                  for c in CASES])
def test_the_record_is_the_twin(R, frame, mount, mask, planar):
    """The mixed batch -- no vehicles; vehicles and no pedestrians; 1, 17, 64, 65, 300 and 1024 rows with 1 .. 9 vehicles; more
    than a tile of points with an own ring across the tile boundary; a ghost and a NaN row; an absent tracked vehicle -- in all
    three split forms (the host file asserts which cases straddle a share boundary)."""
    b, scenes, _ = _batch(R, frame, mount, mask, planar)
    try:
        got = b.vehicle_scans()
        _same(got, VC.twin(scenes, R, frame, mount, mask), "at the upload")
        assert got[0].shape == (0, 2 * R)
        if VC.MASKS[mask][VC.ABSENT[0]] is None:
            assert not got[VC.ABSENT[0]][VC.ABSENT[1]].any()
        splits = {VC.split_of(len(ks) * R) for ks in VC.scanned(scenes, mask) if len(ks)}
        assert splits <= {1, 2, 4}
    finally:
        b.close()


def test_every_split_form_is_run():
    seen = set()
    scenes, _, _ = VC.made()
    for R, _, _, mask, _ in CASES:
        seen |= {VC.split_of(len(ks) * R) for ks in VC.scanned(scenes, mask) if len(ks)}
    assert seen == {1, 2, 4}


def test_a_scene_with_more_vehicles_than_one_chunk():
    """260 small vehicles in one scene: the kernel lists them 256 at a time.  Every vehicle scanned (a full chunk without a split,
    then 4 vehicles x 8 rays shared by 4 waves); two vehicles of each chunk; vehicles of the second chunk only (the first lists
    nobody and is passed over).  A scene of the ordinary kind beside it."""
    import test_batch_gpu as TB
    M, R = 260, 8
    sc = TB._scene(17, 4300, dynamic=M)
    rng = np.random.default_rng(4301)
    c = np.float32(sc["loc"][rng.integers(0, 17, M), :2] + rng.uniform(-6.0, 6.0, (M, 2))).astype(np.float64)
    sc["dynamic_obstacles"] = [(c[j], sc["dynamic_obstacles"][j][1]) for j in range(M)]
    sc["dynamic_extent"] = np.tile([0.3, 0.15], (M, 1))
    V._restart_twin(sc)
    scenes, cfgs, _ = VC.made()
    scenes, cfgs = [sc, scenes[3]], [cfgs[0], cfgs[3]]
    b = V._batch(scenes, cfgs, [0.05, 0.05])
    try:
        for chosen in (None, [3, 255, 256, 259], [257, 258]):
            mask = None if chosen is None else [np.isin(np.arange(M), chosen), [True, True]]
            b.set_vehicle_scan(6.0, 0.3, 0.1, angles=VC.fan(R), mask=mask, frame=1, mount=VC.MOUNT)
            got = b.vehicle_scans()
            want = [S.scan_vehicles_scene(s, VC.fan(R), 6.0, 0.3, 0.1, frame=1, mask=None if mask is None else mask[q], mount=VC.MOUNT)
                    for q, s in enumerate(scenes)]
            _same(got, want, f"vehicles {chosen}")
            assert (got[0][:, R:] == 4).any() and got[0].any(axis=1).sum() == (M if chosen is None else len(chosen))
    finally:
        b.close()


def _tie_batch(scenes, Rmax, ped=0.5, point=0.25):
    cfgs = [V._config(0, V.NO_DYN) for _ in scenes]
    b = SfmBatch(cfgs, [0.05] * len(scenes))
    b.upload(scenes, device_vehicles=True)
    b.set_vehicle_scan(Rmax, ped, point, directions=(np.float32([1, 0, -1, 0]), np.float32([0, 1, 0, -1])))
    return b


def test_designed_ties_on_the_device():
    """The host file's ties, as boxes on the device: a one-point ring is no box, so the candidates stand dead ahead of a real box at
    the same exact range -- a pedestrian disc of radius 0.5 at x + 2, a border and a static point of radius 0.25 at x + 1.75 -- from a
    sensor whose origin has dyadic coordinates; the device and the twin agree on every bit and the earlier kind wins."""
    from carla_social_force_model_amd import scenarios
    local = scenarios.ring_local_offsets(0.5, 0.25)

    def scene(peds, borders=(), statics=(), second=None):
        c = [np.array([8.0, 4.0])] + ([np.asarray(second, np.float64)] if second is not None else [])
        n = len(peds)
        loc = np.hstack([np.asarray(peds, np.float64).reshape(n, 2), np.zeros((n, 1))])
        bl = [np.asarray(p, np.float64).reshape(-1, 2) for p in borders]
        return {"loc": loc, "vel": np.zeros((n, 3)), "waypoint": loc + 1.0, "target_speed": np.ones(n), "radius": np.full(n, 0.3),
                "borders": bl, "border_centers": np.array([p.mean(axis=0) for p in bl]).reshape(-1, 2), "border_lengths": np.ones(len(bl)),
                "static_obstacles": [(np.asarray(p, np.float64).mean(axis=0), np.asarray(p, np.float64).reshape(-1, 2)) for p in statics],
                "dynamic_obstacles": [(ci, scenarios.place_ring_f32(ci, 0.0, local)) for ci in c],
                "dynamic_vel": np.zeros((len(c), 2)), "dynamic_yaw": np.zeros(len(c)), "dynamic_extent": np.array([[0.5, 0.25]] * len(c))}

    pt = [[9.75, 4.0], [9.75, 4.0]]
    scenes = [scene([[10, 4]], borders=[pt]),                             # pedestrian before border
              scene([[10.5, 4]], borders=[pt]),                           # the border alone is nearer
              scene([], borders=[pt], statics=[pt]),                      # border before static
              scene([], statics=[pt]),
              scene([[10, 4], [10, 4]]),                                  # two pedestrians, the same value
              scene([[8.25, 4]])]                                         # the origin inside a pedestrian disc
    want_ray0 = [(1.5, 1), (1.5, 2), (1.5, 2), (1.5, 3), (1.5, 1), (0.0, 1)]
    b = _tie_batch(scenes, 10.0)
    try:
        got = b.vehicle_scans()
        _same(got, [S.scan_vehicles_scene(sc, None, 10.0, 0.5, 0.25, directions=(np.float32([1, 0, -1, 0]), np.float32([0, 1, 0, -1])))
                    for sc in scenes], "ties")
        for s, (r, k) in enumerate(want_ray0):
            assert (got[s][0, 0], got[s][0, 4]) == (np.float32(r), np.float32(k)), s
        assert not (np.concatenate(got)[:, 4:] == 4).any()                 # alone in its scene: the own ring is never reported
    finally:
        b.close()
    b = _tie_batch(scenes[:1], 1.5)                                        # a candidate at exactly Rmax is a miss
    try:
        got = b.vehicle_scans()
        assert (got[0][0, 0], got[0][0, 4]) == (np.float32(1.5), np.float32(0))
    finally:
        b.close()


def test_a_scene_alone_equals_the_scene_in_the_batch():
    R, frame, mount = 33, 1, VC.MOUNT
    b, scenes, tracks = _batch(R, frame, mount, "all")
    try:
        whole = b.vehicle_scans()
    finally:
        b.close()
    _, cfgs, _ = VC.made()
    for s in (1, 5, 6, 8):
        one = V._batch([scenes[s]], [cfgs[s]], [VC.DTS[s]])
        try:
            one.set_vehicle_tracks([tracks[s]])
            one.set_vehicle_scan(VC.RMAX[s], VC.PED[s], VC.POINT[s], angles=VC.fan(R), frame=frame, mount=mount)
            _same(one.vehicle_scans(), [whole[s]], f"scene {s} alone")
        finally:
            one.close()


def _driven(b):
    rng = np.random.default_rng(11)
    kinds = [rng.integers(0, 3, m) for m in VC.COUNTS]
    kinds[VC.ABSENT[0]][VC.ABSENT[1]] = 0                                   # the tracked vehicle follows its track
    cmds = [np.column_stack((rng.uniform(-1.4, 1.4, m), np.cos(rng.uniform(-0.1, 0.1, m)), rng.uniform(-0.1, 0.1, m))).astype(np.float32)
            for m in VC.COUNTS]
    b.set_vehicle_driving(kinds, cmds)
    return kinds, cmds


def _twin_of_device(b, R, frame, mount, mask):
    """The twin fed what the device holds: state, centres, rings and headings, all downloaded."""
    state, veh, drv = b.state(), b.dynamic_obstacles(), b.vehicle_driving()
    return [S.scan_vehicles_scene({"borders": sc["borders"], "static_obstacles": sc["static_obstacles"]}, VC.fan(R), VC.RMAX[s], VC.PED[s],
                                  VC.POINT[s], frame=frame, mask=VC.MASKS[mask][s], mount=mount, state=state[s], vehicles=veh[s],
                                  headings=drv[s][2]) for s, sc in enumerate(VC.made(True)[0])]


def test_scanning_changes_nothing_and_follows_the_moving_parts():
    """State, vehicles, headings, scans() and vehicle_observations() are bitwise the same before and after a vehicle scan; run(3)
    after it equals run(3) without it; after the run with driven vehicles (velocity and unicycle) the record is the twin of the
    downloaded batch; after restart and restart_device it is the snapshot's record again."""
    import torch
    R, frame, mount, mask = 33, 1, VC.MOUNT, "all"
    a, _, _ = _batch(R, frame, mount, mask, finite=True)
    p, _, _ = _batch(R, frame, mount, mask, finite=True, scan=False)
    try:
        for b in (a, p):
            _driven(b)
            b.set_scan(5.0, 0.3, R=8, frame=1)
            b.set_vehicle_observation(4, 6.0, 1)
            b.snapshot()
        everything = lambda b: (V._everything(b), b.vehicle_driving(), b.scans(), b.vehicle_observations())
        before = everything(a)
        first = a.vehicle_scans()
        after = everything(a)
        V._assert_same(before[0], after[0], "before and after a scan")
        for x, y in zip(before[1], after[1]):
            assert all(np.array_equal(u, v) for u, v in zip(x, y))
        for q in (2, 3):
            assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(before[q], after[q]))
        _same(first, _twin_of_device(a, R, frame, mount, mask), "at the snapshot")
        a.scan_vehicles()
        a.run(3)
        a.scan_vehicles()
        p.run(3)
        V._assert_same(V._everything(a), V._everything(p), "run(3) with and without scanning")
        moved = a.vehicle_scans()
        _same(moved, _twin_of_device(a, R, frame, mount, mask), "after run(3), driven")
        assert any((u != v).any() for u, v in zip(moved, first))
        a.restart()
        _same(a.vehicle_scans(), first, "after restart")
        a.run(2)
        done = torch.zeros(a.B, dtype=torch.bool, device="cuda")
        done[[1, 6]] = True
        a.restart_device(done)
        torch.cuda.synchronize()
        got = a.vehicle_scans()
        _same([got[1], got[6]], [first[1], first[6]], "after restart_device")
        _same(got, _twin_of_device(a, R, frame, mount, mask), "after restart_device, every scene")
    finally:
        a.close()
        p.close()


def test_the_tensor_shows_what_the_download_copies():
    import torch
    b, scenes, _ = _batch(8, 0, ZERO, "all")
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        t = b.vehicle_scan_tensor()
        M = sum(VC.COUNTS)
        assert t.shape == (M, 16) and t.dtype == torch.float32 and t.is_cuda
        ptr, nbytes = b.device_ptr(PTR_VEHICLE_SCAN)
        assert t.data_ptr() == ptr and nbytes == M * 16 * 4
        assert not t.any()                                                 # zero-filled by set_vehicle_scan
        got = np.concatenate(b.vehicle_scans())
        assert np.array_equal(t.cpu().numpy().view(np.uint32), got.view(np.uint32)) and got.any()
    finally:
        b.close()


def test_refusals_and_lifetime():
    lib = _lib.load()
    b, scenes, tracks = _batch(8, 0, ZERO, "all")
    f = lambda *v: np.ascontiguousarray(v, dtype=np.float32)
    try:
        B = b.B
        dx, dy = S.ray_directions(VC.fan(8), 256)
        rm, rp, rq = (np.full(B, v, np.float32) for v in (5.0, 0.3, 0.1))
        want = b.vehicle_scans()
        P = lambda a: None if a is None else a.ctypes.data

        def call(R=8, dx=dx, dy=dy, rm=rm, rp=rp, rq=rq, frame=0, mx=0.0, my=0.0):
            return lib.sfm_batch_set_vehicle_scan(b._b, R, P(dx), P(dy), P(rm), P(rp), P(rq), None, frame, mx, my)

        bad = rm.copy()
        bad[3] = np.inf
        big = np.zeros(257, np.float32)
        nan = dx.copy()
        nan[2] = np.nan
        for kw in (dict(R=0), dict(R=257, dx=big, dy=big), dict(frame=2), dict(frame=-1), dict(dx=nan), dict(dy=None), dict(dx=None),
                   dict(rm=bad), dict(rm=np.zeros(B, np.float32)), dict(rp=-rp), dict(rp=None), dict(rq=None), dict(rq=bad),
                   dict(mx=float("nan")), dict(my=float("inf")), dict(mx=2.0e6)):
            assert call(**kw) == -1, kw                                    # SFM_ERR_INVALID
            assert lib.sfm_batch_last_error(b._b)
        _same(b.vehicle_scans(), want, "after the refusals")              # nothing changed: same settings, same buffer
        ptr0 = b.device_ptr(PTR_VEHICLE_SCAN)
        # kept by everything else
        b.set_params([V._config(k, V.ALL) for k in range(B)], VC.DTS)
        b.snapshot()
        b.run(1)
        b.restart()
        b.set_scan(5.0, 0.3, R=4)
        b.set_vehicle_observation(2, 5.0)
        b.set_vehicle_driving(0)
        b.set_vehicle_tracks(tracks)
        assert b.device_ptr(PTR_VEHICLE_SCAN) == ptr0
        _same(b.vehicle_scans(), want, "kept")
        # off: every call gives SFM_ERR_STATE
        b.set_vehicle_scan(None)
        assert lib.sfm_batch_scan_vehicles(b._b) == -3 and lib.sfm_batch_download_vehicle_scan(b._b, None) == -3
        assert not lib.sfm_batch_device_ptr(b._b, PTR_VEHICLE_SCAN, None) and b"vehicle scans are off" in lib.sfm_batch_last_error(b._b)
        with pytest.raises(SfmLibraryError):
            b.vehicle_scan_tensor()
        # dropped by upload; refused without device-side vehicles
        b.set_vehicle_scan(5.0, 0.3, R=8)
        b.upload(scenes)
        assert lib.sfm_batch_scan_vehicles(b._b) == -3
        assert call() == -3                                                # static rings: no device-side vehicles
        with pytest.raises(SfmLibraryError):
            b.set_vehicle_scan(5.0, 0.3, R=8)
        b.upload(scenes, device_vehicles=True)
        assert lib.sfm_batch_scan_vehicles(b._b) == -3                     # ... and not revived by new boxes
        b.set_vehicle_scan(5.0, 0.3, R=256)
        assert np.concatenate(b.vehicle_scans()).shape == (sum(VC.COUNTS), 512)
        # dropped by set_dynamic_boxes alone (the buffer is per vehicle: here scene 6 goes from 9 vehicles to 2) ...
        fewer, _, _ = VC.made()
        for key in ("dynamic_obstacles", "dynamic_vel", "dynamic_yaw", "dynamic_extent", "dynamic_heading", "dynamic_present"):
            fewer[6][key] = fewer[6][key][:2]
        b.set_dynamic_boxes(fewer)
        assert lib.sfm_batch_scan_vehicles(b._b) == -3 and lib.sfm_batch_download_vehicle_scan(b._b, None) == -3
        assert not lib.sfm_batch_device_ptr(b._b, PTR_VEHICLE_SCAN, None)
        b.set_vehicle_scan(VC.RMAX, VC.PED, VC.POINT, angles=VC.fan(33), frame=1, mount=VC.MOUNT)
        got = b.vehicle_scans()
        assert np.concatenate(got).shape == (sum(VC.COUNTS) - 7, 66)
        _same([got[6], got[8]], [S.scan_vehicles_scene(fewer[s], VC.fan(33), VC.RMAX[s], VC.PED[s], VC.POINT[s], frame=1, mount=VC.MOUNT)
                                 for s in (6, 8)], "after new boxes")
        # ... and by sfm_batch_set_dynamic_obstacles alone, after which there are no device-side vehicles to scan
        rings = pack_scenes(fewer)["dynamic"]
        assert lib.sfm_batch_set_dynamic_obstacles(b._b, *(_lib.iptr(a) for a in rings[:2]), *(_lib.fptr(a) for a in rings[2:])) == 0
        assert lib.sfm_batch_scan_vehicles(b._b) == -3 and lib.sfm_batch_download_vehicle_scan(b._b, None) == -3
        assert call() == -3
    finally:
        b.close()
    fresh = SfmBatch([V._config(0, V.ALL)], [0.05])
    try:
        assert lib.sfm_batch_set_vehicle_scan(fresh._b, 8, P(dx), P(dy), P(rm), P(rp), P(rq), None, 0, 0.0, 0.0) == -3   # no state
    finally:
        fresh.close()
