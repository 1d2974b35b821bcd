"""CPU tests of the vehicles' range scan (sfm_batch_set_vehicle_scan, sfm_batch_scan_vehicles; include/sfm_hip.h): what the host twin
scan.scan_vehicles_scene means -- by reduction to scan.scan_scene, which tests/_scan_truth.py ties to a float64 ray cast -- the
designed ties, the classes the GPU file's batch holds, the refusals, and the binding.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import _vehicle_scan_cases as VC
from carla_social_force_model_amd import _lib
from carla_social_force_model_amd import batch as B_
from carla_social_force_model_amd import scan as S
from carla_social_force_model_amd.scan import _fma32, scan_scene, scan_vehicles_scene
from carla_social_force_model_amd.scenarios import vehicle_headings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = (np.float32([1, 0, -1, 0]), np.float32([0, 1, 0, -1]))
AXIS_HEADINGS = np.float32([[1, 0], [0, 1], [-1, 0], [0, -1], [1, 0]])
f32 = np.float32


def _bare(loc, vehicles=(), **more):
    """A scene of pedestrians at ``loc`` and vehicles [(centre, ring points)], everything else empty unless given."""
    loc = np.asarray(loc, dtype=np.float64).reshape(-1, 2)
    n = len(loc)
    sc = {"loc": np.hstack([loc, np.zeros((n, 1))]), "vel": np.zeros((n, 3)), "waypoint": np.hstack([loc + 1.0, np.zeros((n, 1))]),
          "target_speed": np.ones(n), "dynamic_obstacles": [(np.asarray(c, np.float64), np.asarray(r, np.float64).reshape(-1, 2))
                                                            for c, r in vehicles],
          "dynamic_yaw": np.zeros(len(vehicles))}
    sc.update(more)
    return sc


def _scan1(sc, Rmax=10.0, ped=0.5, point=0.25, **kw):
    kw.setdefault("directions", AXES)
    return scan_vehicles_scene(sc, None, Rmax, ped, point, **kw)


# ---- the twin's meaning: vehicle k's record is scan_scene's record of a probe row at the sensor's origin, with k taken out ---------

def _by_scan_scene(sc, k, dirs, Rmax, ped, point, mount, frame, h):
    c = f32(sc["dynamic_obstacles"][k][0])
    hx, hy = f32(h[k])
    mx, my = f32(mount)
    ox = f32(c[0] + _fma32(hx, mx, -(hy * my))[()])                     # the origin, by the rules
    oy = f32(c[1] + _fma32(hy, mx, hx * my)[()])
    n = len(sc["loc"])
    row = lambda a, b: np.vstack([np.asarray(a, dtype=np.float64).reshape(n, 3), [[b[0], b[1], 0.0]]])
    probe = dict(sc, loc=row(sc["loc"], (ox, oy)), vel=row(sc["vel"], (hx, hy) if frame else (0.0, 0.0)),
                 waypoint=row(sc["waypoint"], (ox, oy)), target_speed=np.append(sc["target_speed"], 1.0),
                 dynamic_obstacles=[v for j, v in enumerate(sc["dynamic_obstacles"]) if j != k])
    mask = np.zeros(n + 1, bool)
    mask[n] = True
    return scan_scene(probe, None, Rmax, ped, point, frame=frame, mask=mask, directions=dirs)[n]


@pytest.mark.parametrize("mount", [(0.0, 0.0), VC.MOUNT], ids=["centre", "front"])
@pytest.mark.parametrize("m", [1, 3, 5])
def test_the_twin_reduces_to_the_row_scan(m, mount):
    """Every vehicle k of scenes with 1, 3 and 5 vehicles: frame 0 at the scene's own headings, and frame 1 with headings on the four
    axes, where the probe row's velocity along the heading makes scan.heading32 reproduce the heading exactly."""
    s = VC.COUNTS.index(m)
    sc = VC.made()[0][s]
    dirs = S.ray_directions(VC.fan(33))
    for frame, h in ((0, vehicle_headings(sc)), (1, AXIS_HEADINGS[:m])):
        rec = scan_vehicles_scene(sc, None, VC.RMAX[s], VC.PED[s], VC.POINT[s], frame=frame, mount=mount, headings=h, directions=dirs)
        assert rec.shape == (m, 66) and rec.dtype == np.float32
        for k in range(m):
            want = _by_scan_scene(sc, k, dirs, VC.RMAX[s], VC.PED[s], VC.POINT[s], mount, frame, h)
            assert np.array_equal(rec[k].view(np.uint32), want.view(np.uint32)), (frame, k)
        assert (rec[:, 33:] > 0).any() and (m == 1 or (rec[:, 33:] == 0).any())    # something is hit, something is missed
        assert np.array_equal(rec, scan_vehicles_scene(sc, None, VC.RMAX[s], VC.PED[s], VC.POINT[s], frame=frame, mount=mount,
                                                       headings=h, directions=dirs, prune=False))


# ---- what the GPU file's batch holds, from the twin alone -------------------------------------------------------------------------

def test_classes_held_by_the_batch():
    scenes, _, _ = VC.made()
    assert [len(sc["loc"]) for sc in scenes] == list(VC.SIZES) and [len(sc["dynamic_obstacles"]) for sc in scenes] == list(VC.COUNTS)
    R = 33
    recs = VC.twin(scenes, R, 0, (0.0, 0.0), "all")
    kinds = np.concatenate([r[:, R:].ravel() for r in recs])
    ranges = np.concatenate([r[:, :R].ravel() for r in recs])
    assert {0.0, 1.0, 2.0, 3.0, 4.0} <= set(kinds.tolist())               # a miss and a hit of each kind
    assert ((ranges == 0) & (kinds == 1)).any()                            # an origin inside a pedestrian disc
    assert not recs[VC.ABSENT[0]][VC.ABSENT[1]].any() and recs[VC.ABSENT[0]][0].any()     # the absent tracked vehicle reads zeros
    assert (recs[1][:, R:] == 4).any() and set(recs[1][:, R:].ravel().tolist()) <= {0.0, 4.0}   # no crowd, no borders: the other vehicle
    assert recs[0].shape == (0, 2 * R)                                     # a scene without vehicles
    masked = VC.twin(scenes, R, 0, (0.0, 0.0), "middle")
    assert not masked[6][0].any() and np.array_equal(masked[6][4], recs[6][4]) and np.array_equal(masked[6][5], recs[6][5])
    # kind 4 is never the vehicle's own ring: alone in its scene a vehicle reports none (next test), and in the batch every kind-4
    # hit of vehicle k is one of scan_scene's hits with k taken out (the reduction above)
    sc = scenes[5]                                                         # the ghost and the NaN row are nobody's hit
    assert not np.isfinite(sc["loc"][VC.NAN_ROW, 0]) and abs(sc["loc"][VC.GHOST, 0]) > 1e12
    assert np.isfinite(recs[5]).all()


def test_the_batch_straddles_tiles_and_shares():
    """The index arithmetic of the kernel, restated: scene 8 has more than a tile of points in front of the rings and vehicle 0's own
    ring lies across the tile boundary; with 9 vehicles another ring does; and among the cases the GPU file runs (CASES), for a split
    of 4 and of 2 some scanned vehicle's own ring lies across the boundary between two waves' shares, and both tile straddlers are
    scanned."""
    scenes, _, _ = VC.made()
    nb, ns, rings = VC.counts(scenes[8])
    assert nb + ns < VC.TILE < nb + ns + rings[0] and nb + ns + sum(rings) > VC.TILE and VC.straddles_tile(scenes[8], 0)
    assert any(VC.straddles_tile(scenes[6], k) for k in range(9))
    seen = set()
    tiles = set()
    assert {c[0] for c in VC.CASES} == set(VC.RAYS) and {c[3] for c in VC.CASES} == set(VC.MASKS)
    for R, _, _, mask, _ in VC.CASES:
        for s, ks in enumerate(VC.scanned(scenes, mask)):
            split = VC.split_of(len(ks) * R)
            seen.add((split, any(split > 1 and VC.straddles_share(scenes[s], k, split, VC.POINT[s]) for k in ks)))
            tiles |= {(s, int(k)) for k in ks if VC.straddles_tile(scenes[s], k)}
    assert {(4, True), (2, True), (1, False)} <= seen
    assert (8, 0) in tiles and any(s == 6 for s, _ in tiles)


def test_the_own_ring_is_left_out():
    ring = [[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]]              # dead ahead on every axis ray
    alone = _bare([], [((0, 0), ring)])
    rec = _scan1(alone, ped=0.0)
    assert np.array_equal(rec, f32([[10, 10, 10, 10, 0, 0, 0, 0]]))
    two = _bare([], [((0, 0), ring), ((5, 0), [[4.0, 0.0], [6.0, 0.0]])])
    rec = _scan1(two, ped=0.0)
    assert np.array_equal(rec[0], f32([3.75, 10, 10, 10, 4, 0, 0, 0]))     # the other vehicle's ring point at (4, 0)
    # from (5, 0): its own (6, 0) and (4, 0), both 0.75 away, are skipped; behind it vehicle 0's (1, 0) at 4 - 0.25
    assert np.array_equal(rec[1], f32([10, 10, 3.75, 10, 0, 0, 4, 0]))


def test_designed_ties():
    """Dyadic numbers on axis rays (c = 0, w exact): equal ranges go to the earlier candidate of the fixed order; the vehicle's own ring
    point at (1, 0), nearer than everything, is never taken."""
    own = ((0, 0), [[1.0, 0.0]])
    pt = np.array([[1.75, 0.0]])
    other = ((9, 9), pt)
    ped_border = _bare([[2, 0]], [own], borders=[pt])
    assert np.array_equal(_scan1(ped_border)[0, [0, 4]], f32([1.5, 1]))                       # pedestrian before border
    assert np.array_equal(_scan1(_bare([[2.5, 0]], [own], borders=[pt]))[0, [0, 4]], f32([1.5, 2]))
    border_static = _bare([], [own], borders=[pt], static_obstacles=[((0, 0), pt)])
    assert np.array_equal(_scan1(border_static)[0, [0, 4]], f32([1.5, 2]))                    # border before static
    static_vehicle = _bare([], [own, other], static_obstacles=[((0, 0), pt)])
    assert np.array_equal(_scan1(static_vehicle)[0, [0, 4]], f32([1.5, 3]))                   # static before another vehicle's ring
    assert np.array_equal(_scan1(_bare([], [own, other]))[0, [0, 4]], f32([1.5, 4]))
    assert np.array_equal(_scan1(_bare([], [other, own]))[1, [0, 4]], f32([1.5, 4]))          # ... whichever comes first
    two_peds = _bare([[2, 0], [2, 0]], [own])
    assert np.array_equal(_scan1(two_peds)[0, [0, 4]], f32([1.5, 1]))                         # the lower row first: the same value
    assert np.array_equal(_scan1(ped_border, Rmax=1.5)[0, [0, 4]], f32([1.5, 0]))             # a candidate at exactly Rmax is a miss
    assert np.array_equal(_scan1(ped_border, Rmax=1.75)[0, [0, 4]], f32([1.5, 1]))
    inside = _bare([[0.25, 0]], [own])
    rec = _scan1(inside)                                                                      # origin inside a pedestrian disc
    assert np.array_equal(rec[0], f32([0, 0, 0, 0, 1, 1, 1, 1])) and not np.signbit(rec[0, :4]).any()


def test_mount_frame_mask_and_absence():
    h = f32([[0, 1]])                                                      # the vehicle looks along +y
    sc = _bare([[0, 5]], [((0, 0), [[0.0, 2.0]])])
    rec = _scan1(sc, headings=h, frame=1)                                  # ray 0 (forward) is +y in the world
    assert np.array_equal(rec[0], f32([4.5, 10, 10, 10, 1, 0, 0, 0]))
    rec = _scan1(sc, headings=h, frame=1, mount=(2.0, 0.0))                # two metres further forward
    assert np.array_equal(rec[0], f32([2.5, 10, 10, 10, 1, 0, 0, 0]))
    rec = _scan1(sc, headings=h, frame=0, mount=(2.0, 0.0))                # world axes: ray 1 is +y
    assert np.array_equal(rec[0], f32([10, 2.5, 10, 10, 0, 1, 0, 0]))
    rec = _scan1(sc, headings=h, mount=(0.0, -3.0))                        # three metres to the right of +y: at (3, 0)
    assert np.array_equal(rec[0], f32([10, 10, 10, 10, 0, 0, 0, 0]))
    two = _bare([[0, 5]], [((0, 0), []), ((np.inf, np.inf), [[np.inf, np.inf]])])
    rec = _scan1(two, mask=[True, True])
    assert rec[0].any() and not rec[1].any()                               # an absent vehicle: zeros
    assert not _scan1(two, mask=[False, True]).any()                       # masked out: zeros
    three_d = dict(sc, loc=sc["loc"] + [0, 0, 7.0])
    assert np.array_equal(_scan1(three_d, headings=h), _scan1(sc, headings=h))          # only x and y are used
    assert _scan1(_bare([], [])).shape == (0, 8)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_twin_and_the_packers():
    sc = _bare([[2, 0]], [((0, 0), [[1.0, 0.0]]), ((5, 5), [[5.0, 5.0]])])
    io = np.int32([0, 2])
    ok = dict(angles=VC.fan(8), max_range=5.0, ped_radius=0.3, point_radius=0.1)
    assert scan_vehicles_scene(sc, **ok).shape == (2, 16)
    assert scan_vehicles_scene(sc, **dict(ok, angles=VC.fan(256))).shape == (2, 512)
    bad = [dict(angles=np.zeros(0)), dict(angles=VC.fan(257)), dict(frame=2), dict(angles=[0.0, np.nan]), dict(max_range=np.inf),
           dict(max_range=0.0), dict(max_range=2.0e6), dict(ped_radius=-1.0), dict(ped_radius=np.nan), dict(point_radius=np.inf),
           dict(mount=(np.nan, 0.0)), dict(mount=(0.0, 2.0e6)), dict(mount=(1.0,)), dict(mask=[True]), dict(mask=np.ones((2, 1), bool)),
           dict(angles=None, directions=(np.ones(257), np.ones(257))), dict(angles=None, directions=([np.inf], [0.0]))]
    for kw in bad:
        with pytest.raises(ValueError):
            scan_vehicles_scene(sc, **dict(ok, **kw))
    for R in (0, 257):
        with pytest.raises(ValueError):
            S.default_angles(R, S.MAX_VEHICLE_SCAN_RAYS)
    assert S.default_angles(256, S.MAX_VEHICLE_SCAN_RAYS).shape == (256,) and S.MAX_VEHICLE_SCAN_RAYS == 256
    rm, rp, rq, mk, frame, mx, my = B_.vehicle_scan_arrays(io, 5.0, 0.3, 0.1, 1, [[True, False]], (1.0, -0.5))
    assert rm.dtype == np.float32 and rm.shape == (1,) and np.array_equal(mk, np.uint8([1, 0])) and frame == 1 and (mx, my) == (1.0, -0.5)
    assert B_.vehicle_scan_arrays(io, 5.0, 0.3)[3] is None
    for kw in (dict(frame=2), dict(max_range=np.nan), dict(ped_radius=-0.1), dict(point_radius=2.0e6), dict(mount=(np.inf, 0.0)),
               dict(mask=[[True]]), dict(mask=np.ones(3, bool)), dict(max_range=[5.0, 5.0])):
        args = dict(dict(max_range=5.0, ped_radius=0.3, point_radius=0.1), **kw)
        with pytest.raises(ValueError):
            B_.vehicle_scan_arrays(io, **args)


def test_the_row_scan_keeps_its_64_rays():
    assert S.MAX_SCAN_RAYS == 64 and S.default_angles(64).shape == (64,)
    for call in (lambda: S.default_angles(65), lambda: S.ray_directions(np.zeros(65)), lambda: S.check_directions((np.ones(65), np.ones(65))),
                 lambda: scan_scene(_bare([[0, 0]]), np.zeros(65), 5.0, 0.3, 0.1)):
        with pytest.raises(ValueError):
            call()
    assert S.ray_directions(np.zeros(65), 256)[0].shape == (65,) and S.check_directions((np.ones(65), np.ones(65)), 256)[0].shape == (65,)


# ---- binding and header --------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert int(re.search(r"#define SFM_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 17
    names = ("sfm_batch_set_vehicle_scan", "sfm_batch_scan_vehicles", "sfm_batch_download_vehicle_scan")
    for name in names:
        assert name in _lib.SYMBOLS and _lib.SINCE[name] == 17 and name in _lib.UNBUMPED
        assert re.search(r"^int " + name + r"\(SfmBatch\* b", header, re.M), name
    assert [len(_lib.SYMBOLS[n][1]) for n in names] == [11, 1, 2]
    for name, val in (("SFM_BATCH_PTR_VEHICLE_SCAN", B_.PTR_VEHICLE_SCAN), ("SFM_BATCH_MAX_VEHICLE_SCAN_RAYS", S.MAX_VEHICLE_SCAN_RAYS)):
        assert re.search(r"#define " + name + r" " + str(val) + r"\b", header), name
    assert B_.PTR_VEHICLE_SCAN == 12
    lib = _lib.load()                                                      # bound: the built library exports them
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
    usage = open(os.path.join(ROOT, "carla-social-force-model_amd", "csrc", "resource_usage.txt")).read()
    block = usage[usage.index("sfm_batch_vehicle_scan_kernel"):]
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", block[:block.index("LDS Size")])


def test_the_lidar_example_imports_and_its_policy_reads_the_scan():
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("batch_av_lidar_loop", os.path.join(ROOT, "examples", "batch_av_lidar_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    R = 9
    dirs = torch.as_tensor(np.stack(S.ray_directions(ex.fan_angles(R), 256), axis=1))
    free = torch.full((2, R), ex.MAX_RANGE)
    cmd = ex.policy(free, dirs)
    assert cmd.shape == (2, 3) and torch.allclose(cmd[:, 0], torch.full((2,), ex.CRUISE)) and torch.allclose(cmd[:, 2], torch.zeros(2), atol=1e-6)
    near = free.clone()
    near[0, R // 2] = 1.0                                                  # something one metre dead ahead of vehicle 0: it brakes
    braked = ex.policy(near, dirs)
    assert braked[0, 0] < cmd[0, 0] and torch.equal(braked[1], cmd[1])
