"""GPU tests of the vehicles' bird's-eye grid (sfm_batch_set_vehicle_grid, sfm_batch_grid_vehicles, sfm_batch_download_vehicle_grid;
SfmBatch.set_vehicle_grid / grid_vehicles / vehicle_grids / vehicle_grid_items / vehicle_grid_tensor): the record against the host
twin grid.grid_vehicles_scene BIT FOR BIT -- there is no tolerance anywhere -- on the batch of tests/_vehicle_grid_cases.py, which
test_batch_vehicle_grid_host.py ties to a float64 statement.  Run on the MI355X box with  python -m pytest tests -m gpu."""
import numpy as np
import pytest

import _vehicle_grid_cases as VG
import test_batch_vehicles_gpu as V
from carla_social_force_model_amd import _lib, grid as G
from carla_social_force_model_amd.batch import PTR_VEHICLE_GRID, SfmBatch, SfmLibraryError, pack_scenes

pytestmark = pytest.mark.gpu

ZERO, FORWARD, CASES = VG.ZERO, VG.FORWARD, VG.CASES


def _batch(GU, GV, scale, frame, centre, mask, planar=None, finite=False, grid=True):
    scenes, cfgs, tracks = VG.made(finite)
    b = V._batch(scenes, cfgs, VG.DTS, planar)
    try:
        b.set_vehicle_tracks(tracks)
        if grid:
            b.set_vehicle_grid(VG.cells_of(scale), GU, GV, mask=VG.mask_arg(mask), frame=frame, centre=centre)
    except Exception:
        b.close()
        raise
    return b, scenes, tracks


def _same(got, want, what):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.float32, f"{what}: scene {s} shape {g.shape} for {w.shape}"
        gb, wb = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(gb, wb), f"{what}: scene {s}, (slot, channel) {np.argwhere((gb != wb).any(axis=(2, 3))).tolist()[:8]}"


@pytest.mark.parametrize("GU,GV,scale,frame,centre,mask,planar", CASES,
                         ids=[f"{c[0]}x{c[1]}-f{c[3]}-{'m' if c[4] != ZERO else 'c'}-{c[5]}-{'3d' if c[6] is False else 'xy'}" for c in CASES])
def test_the_record_is_the_twin(GU, GV, scale, frame, centre, mask, planar):
    """The mixed batch -- no vehicles; vehicles and no pedestrians; 1, 255, 256, 257 and 1 024 rows with 1, 2, 3, 9 and 70 vehicles;
    geometry beyond the LDS tile; more ring points of other vehicles than one list chunk; an own ring across the tile boundary; a
    ghost and a NaN row; an absent tracked vehicle -- with the buffer filled with NaN before the launch."""
    import torch
    b, scenes, _ = _batch(GU, GV, scale, frame, centre, mask, planar)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        items = b.vehicle_grid_items()
        want_items = G.vehicle_grid_slots(VG.mask_arg(mask), b._dyn[0])[0]
        assert np.array_equal(items, want_items)
        t = b.vehicle_grid_tensor()
        assert t.shape == (len(items), 8, GV, GU)
        t.fill_(float("nan"))                                             # every float of every slot is rewritten
        got = b.vehicle_grids()
        _same(got, VG.twin(scenes, GU, GV, scale, frame, centre, mask), "at the upload")
        assert got[0].shape == (0, 8, GV, GU) and not np.isnan(np.concatenate(got)).any()
        if mask == "all":
            assert not got[VG.ABSENT[0]][VG.ABSENT[1]].any()
            if GU * GV > 1:
                assert all(np.concatenate(got)[:, ch].any() for ch in range(8))
        if mask == "middle":
            assert got[3].shape[0] == 0 and got[6].shape[0] == 0 and got[4].shape[0] == 1
    finally:
        b.close()


def _hand_batch(scenes):
    cfgs = [V._config(0, V.NO_DYN) for _ in scenes]
    b = SfmBatch(cfgs, [0.05] * len(scenes))
    b.upload(scenes, device_vehicles=True)
    return b


@pytest.mark.parametrize("frame", [0, 1])
def test_the_sum_orders_on_the_device(frame):
    """The mixed-magnitude cases of the host file: 1, -2^25, 2^25 in one cell, forwards and backwards, as pedestrians and as vehicles."""
    scenes = [VG.order_scene_pedestrians(), VG.order_scene_pedestrians(VG.ORDER_VALUES[::-1]),
              VG.order_scene_vehicles(), VG.order_scene_vehicles(VG.ORDER_VALUES[::-1])]
    b = _hand_batch(scenes)
    try:
        b.set_vehicle_grid(1.0, 8, 8, frame=frame)
        got = b.vehicle_grids()
        _same(got, [G.grid_vehicles_scene(sc, 8, 8, 1.0, frame=frame) for sc in scenes], "orders")
        p = len(scenes[2]["dynamic_obstacles"][1][1])
        assert got[0][0, 1, 4, 6] == 0 and got[1][0, 1, 4, 6] == 1 and got[0][0, 0, 4, 6] == 3
        assert got[2][0, 5, 4, 6] == 3 * p
        assert got[2][0, 6, 4, 6] == VG.ordered([v for v in VG.ORDER_VALUES for _ in range(p)])
        assert got[3][0, 6, 4, 6] == VG.ordered([v for v in VG.ORDER_VALUES[::-1] for _ in range(p)])
        assert not got[0][0, 5:].any()                                    # a lone vehicle: its own ring is never counted
    finally:
        b.close()


def test_a_scene_alone_equals_the_scene_in_the_batch():
    GU, GV, scale, frame, centre = 33, 8, 1.0, 1, FORWARD
    b, scenes, tracks = _batch(GU, GV, scale, frame, centre, "all")
    try:
        whole = b.vehicle_grids()
    finally:
        b.close()
    _, cfgs, _ = VG.made()
    for s in (1, 4, 5, 7, 8):
        one = V._batch([scenes[s]], [cfgs[s]], [VG.DTS[s]])
        try:
            one.set_vehicle_tracks([tracks[s]])
            one.set_vehicle_grid(VG.cells_of(scale)[s], GU, GV, frame=frame, centre=centre)
            _same(one.vehicle_grids(), [whole[s]], f"scene {s} alone")
        finally:
            one.close()
    # ... and anywhere in another batch: the scenes in reverse order
    order = list(range(len(scenes)))[::-1]
    rev = V._batch([scenes[s] for s in order], [cfgs[s] for s in order], [VG.DTS[s] for s in order])
    try:
        rev.set_vehicle_tracks([tracks[s] for s in order])
        rev.set_vehicle_grid([VG.cells_of(scale)[s] for s in order], GU, GV, frame=frame, centre=centre)
        _same(rev.vehicle_grids(), [whole[s] for s in order], "reversed")
    finally:
        rev.close()


def _driven(b):
    rng = np.random.default_rng(12)
    kinds = [rng.integers(0, 3, m) for m in VG.COUNTS]
    kinds[VG.ABSENT[0]][VG.ABSENT[1]] = 0                                   # the tracked vehicle follows its track
    cmds = [np.column_stack((rng.uniform(-1.4, 1.4, m), np.cos(rng.uniform(-0.1, 0.1, m)), rng.uniform(-0.1, 0.1, m))).astype(np.float32)
            for m in VG.COUNTS]
    b.set_vehicle_driving(kinds, cmds)
    return kinds, cmds


def _twin_of_device(b, GU, GV, scale, frame, centre, mask):
    """The twin fed what the device holds: state, centres, rings, headings and velocities, all downloaded."""
    state, veh, drv = b.state(), b.dynamic_obstacles(), b.vehicle_driving()
    base = [{"borders": sc["borders"], "static_obstacles": sc["static_obstacles"]} for sc in VG.made(True)[0]]
    return VG.twin(base, GU, GV, scale, frame, centre, mask, state=state, vehicles=veh, headings=[d[2] for d in drv],
                   vehicle_vel=[d[3] for d in drv])


def test_gridding_changes_nothing_and_follows_the_moving_parts():
    """State, vehicles, headings, scans(), vehicle_scans(), grids() and vehicle_observations() are bitwise the same before and after
    a vehicle grid; run(3) after it equals run(3) without it; after the run with driven vehicles (velocity and unicycle) and after
    the keyframe teleport of the tracked vehicle the record is the twin of the downloaded batch; after restart and restart_device it
    is the snapshot's record again."""
    import torch
    GU, GV, scale, frame, centre, mask = 33, 8, 1.0, 1, FORWARD, "all"
    a, _, _ = _batch(GU, GV, scale, frame, centre, mask, finite=True)
    p, _, _ = _batch(GU, GV, scale, frame, centre, mask, finite=True, grid=False)
    try:
        for b in (a, p):
            _driven(b)
            b.set_scan(5.0, 0.3, R=8, frame=1)
            b.set_vehicle_scan(6.0, 0.3, R=8, frame=1)
            b.set_grid(0.5, G=8, frame=1)
            b.set_vehicle_observation(4, 6.0, 1)
            b.snapshot()
        everything = lambda b: (V._everything(b), b.vehicle_driving(), b.scans(), b.vehicle_scans(), b.grids(), b.vehicle_observations())
        before = everything(a)
        first = a.vehicle_grids()
        after = everything(a)
        V._assert_same(before[0], after[0], "before and after a grid")
        for x, y in zip(before[1], after[1]):
            assert all(np.array_equal(u, v) for u, v in zip(x, y))
        for q in (2, 3, 4, 5):
            assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(before[q], after[q]))
        _same(first, _twin_of_device(a, GU, GV, scale, frame, centre, mask), "at the snapshot")
        a.grid_vehicles()
        a.run(3)
        a.grid_vehicles()
        p.run(3)
        V._assert_same(V._everything(a), V._everything(p), "run(3) with and without gridding")
        moved = a.vehicle_grids()
        _same(moved, _twin_of_device(a, GU, GV, scale, frame, centre, mask), "after run(3), driven")
        assert any((u != v).any() for u, v in zip(moved, first))
        a.run(40)                                                          # the tracked vehicle has arrived: a keyframe teleport
        assert np.isfinite(a.dynamic_obstacles()[VG.ABSENT[0]][VG.ABSENT[1]][0]).all()
        arrived = a.vehicle_grids()
        _same(arrived, _twin_of_device(a, GU, GV, scale, frame, centre, mask), "after the teleport")
        assert arrived[VG.ABSENT[0]][VG.ABSENT[1]].any()
        a.restart()
        _same(a.vehicle_grids(), first, "after restart")
        a.run(2)
        done = torch.zeros(a.B, dtype=torch.bool, device="cuda")
        done[[1, 7]] = True
        a.restart_device(done)
        torch.cuda.synchronize()
        got = a.vehicle_grids()
        _same([got[1], got[7]], [first[1], first[7]], "after restart_device")
        _same(got, _twin_of_device(a, GU, GV, scale, frame, centre, mask), "after restart_device, every scene")
    finally:
        a.close()
        p.close()


def test_the_tensor_shows_what_the_download_copies():
    import torch
    b, scenes, _ = _batch(17, 15, 1.0, 0, ZERO, "first")
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        t = b.vehicle_grid_tensor()
        M = sum(1 for m in VG.COUNTS if m)
        assert t.shape == (M, 8, 15, 17) and t.dtype == torch.float32 and t.is_cuda
        ptr, nbytes = b.device_ptr(PTR_VEHICLE_GRID)
        assert t.data_ptr() == ptr and nbytes == M * 8 * 15 * 17 * 4
        assert not t.any()                                                 # zero-filled by set_vehicle_grid
        got = np.concatenate(b.vehicle_grids())
        assert np.array_equal(t.cpu().numpy().view(np.uint32), got.view(np.uint32)) and got.any()
        # no gridded vehicle: on, no buffer, nothing launched
        b.set_vehicle_grid(0.5, 8, 8, mask=[np.zeros(m, bool) for m in VG.COUNTS])
        assert b.device_ptr(PTR_VEHICLE_GRID) == (0, 0) and b.vehicle_grid_tensor().shape == (0, 8, 8, 8)
        assert all(g.shape == (0, 8, 8, 8) for g in b.vehicle_grids()) and len(b.vehicle_grid_items()) == 0
    finally:
        b.close()


def test_refusals_and_lifetime():
    lib = _lib.load()
    GU, GV, scale, frame, centre = 16, 16, 1.0, 1, FORWARD
    b, scenes, tracks = _batch(GU, GV, scale, frame, centre, "all")
    try:
        B = b.B
        cell = np.full(B, 0.5, np.float32)
        want = b.vehicle_grids()
        P = lambda a: None if a is None else a.ctypes.data
        unknown = lambda: lib.sfm_batch_last_error(b._b)

        def call(GU=8, GV=8, cell=cell, frame=0, cx=0.0, cy=0.0):
            return lib.sfm_batch_set_vehicle_grid(b._b, GU, GV, P(cell), None, frame, cx, cy)

        bad = cell.copy()
        bad[3] = np.inf
        for kw in (dict(GU=0), dict(GU=65), dict(GV=0), dict(GV=65), dict(GU=33, GV=32), dict(GU=64, GV=17), dict(frame=2), dict(frame=-1),
                   dict(cell=bad), dict(cell=np.zeros(B, np.float32)), dict(cell=-cell), dict(cell=np.full(B, 2.0e6, np.float32)),
                   dict(cell=np.full(B, np.nan, np.float32)), dict(cx=float("nan")), dict(cy=float("inf")), dict(cx=2.0e6), dict(cy=-2.0e6)):
            assert call(**kw) == -1, kw                                    # SFM_ERR_INVALID
            assert lib.sfm_batch_last_error(b._b)
        with pytest.raises(ValueError):
            b.set_vehicle_grid(0.5, 33, 32)
        _same(b.vehicle_grids(), want, "after the refusals")              # nothing changed: same settings, same buffer
        ptr0 = b.device_ptr(PTR_VEHICLE_GRID)
        assert ptr0[1] == sum(VG.COUNTS) * 8 * GU * GV * 4
        # kept by everything else
        b.set_params([V._config(k, V.ALL) for k in range(B)], VG.DTS)
        b.snapshot()
        b.run(1)
        b.restart()
        b.set_scan(5.0, 0.3, R=4)
        b.set_grid(0.5, G=4)
        b.set_vehicle_scan(5.0, 0.3, R=4)
        b.set_vehicle_observation(2, 5.0)
        b.set_vehicle_driving(0)
        b.set_vehicle_tracks(tracks)
        assert b.device_ptr(PTR_VEHICLE_GRID) == ptr0
        _same(b.vehicle_grids(), want, "kept")
        # off: launch and download give SFM_ERR_STATE, the pointer value is the unknown value it was
        lib.sfm_batch_device_ptr(b._b, 99, None)
        message = unknown()
        b.set_vehicle_grid(None)
        assert lib.sfm_batch_grid_vehicles(b._b) == -3 and lib.sfm_batch_download_vehicle_grid(b._b, None) == -3
        assert b"vehicle grids are off" in unknown()
        assert not lib.sfm_batch_device_ptr(b._b, PTR_VEHICLE_GRID, None) and unknown() == message
        for f in (b.vehicle_grid_tensor, b.vehicle_grids, b.vehicle_grid_items, b.grid_vehicles):
            with pytest.raises(SfmLibraryError):
                f()
        # dropped by upload; refused without device-side vehicles
        b.set_vehicle_grid(0.5, 8, 8)
        b.upload(scenes)
        assert lib.sfm_batch_grid_vehicles(b._b) == -3
        assert call() == -3                                                # static rings: no device-side vehicles
        with pytest.raises(SfmLibraryError):
            b.set_vehicle_grid(0.5, 8, 8)
        b.upload(scenes, device_vehicles=True)
        assert lib.sfm_batch_grid_vehicles(b._b) == -3                     # ... and not revived by new boxes
        b.set_vehicle_grid(0.5, 64, 16)
        assert np.concatenate(b.vehicle_grids()).shape == (sum(VG.COUNTS), 8, 16, 64)
        # dropped by set_dynamic_boxes alone (the buffer is per vehicle: here scene 4 goes from 9 vehicles to 2) ...
        fewer, _, _ = VG.made()
        for key in ("dynamic_obstacles", "dynamic_vel", "dynamic_yaw", "dynamic_extent", "dynamic_heading", "dynamic_present"):
            fewer[4][key] = fewer[4][key][:2]
        b.set_dynamic_boxes(fewer)
        assert lib.sfm_batch_grid_vehicles(b._b) == -3 and lib.sfm_batch_download_vehicle_grid(b._b, None) == -3
        assert not lib.sfm_batch_device_ptr(b._b, PTR_VEHICLE_GRID, None) and unknown() == message
        b.set_vehicle_grid(VG.cells_of(1.0), 17, 15, frame=1, centre=FORWARD)
        got = b.vehicle_grids()
        assert np.concatenate(got).shape == (sum(VG.COUNTS) - 7, 8, 15, 17)
        _same([got[4], got[8]], [G.grid_vehicles_scene(fewer[s], 17, 15, VG.CELLS[s], frame=1, centre=FORWARD) for s in (4, 8)], "after new boxes")
        # ... and by sfm_batch_set_dynamic_obstacles alone, after which there are no device-side vehicles to grid
        rings = pack_scenes(fewer)["dynamic"]
        assert lib.sfm_batch_set_dynamic_obstacles(b._b, *(_lib.iptr(a) for a in rings[:2]), *(_lib.fptr(a) for a in rings[2:])) == 0
        assert lib.sfm_batch_grid_vehicles(b._b) == -3 and lib.sfm_batch_download_vehicle_grid(b._b, None) == -3
        assert call() == -3
    finally:
        b.close()
    fresh = SfmBatch([V._config(0, V.ALL)], [0.05])
    try:
        assert lib.sfm_batch_set_vehicle_grid(fresh._b, 8, 8, P(cell), None, 0, 0.0, 0.0) == -3   # no state
        assert lib.sfm_batch_grid_vehicles(fresh._b) == -3
    finally:
        fresh.close()


def test_a_batch_that_has_been_through_another_crowd():
    """A batch that gridded a larger crowd with more vehicles, then uploads the mixed batch's first scenes: it reads back what a
    fresh batch reads back."""
    scenes, cfgs, tracks = VG.made()
    pick = [6, 7, 1]
    big = [scenes[s] for s in pick]
    small = [scenes[s] for s in (3, 5, 2)]
    b = V._batch(big, [cfgs[s] for s in pick], [0.05] * 3)
    try:
        b.set_vehicle_grid(0.5, 64, 16, frame=1, centre=FORWARD)
        assert np.concatenate(b.vehicle_grids()).any()
        b.upload(small, device_vehicles=True)
        b.set_vehicle_grid(0.5, 17, 15, frame=1, centre=FORWARD, mask=[[1, 0], [0, 1, 1], None])
        got = b.vehicle_grids()
    finally:
        b.close()
    f = V._batch(small, [cfgs[s] for s in pick], [0.05] * 3)
    try:
        f.set_vehicle_grid(0.5, 17, 15, frame=1, centre=FORWARD, mask=[[1, 0], [0, 1, 1], None])
        _same(got, f.vehicle_grids(), "fresh")
        assert [len(g) for g in got] == [1, 2, 1] and np.concatenate(got).any()
    finally:
        f.close()


def test_the_example_runs():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "batch_av_grid_loop.py")
    spec = importlib.util.spec_from_file_location("batch_av_grid_loop", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    episodes, arrivals, hits = mod.run(B=8, steps=6, repeat=2, quiet=True)
    assert episodes >= arrivals + hits >= 0
