"""GPU tests of occupancy grids on a batch (sfm_batch_set_grid, sfm_batch_grid, sfm_batch_download_grid, SFM_BATCH_PTR_GRID;
SfmBatch.set_grid / grid / grids / grid_rows / grid_tensor): bitwise against the host twin ``grid.grid_scene`` in BOTH frames, the
compact slots, independence of the rest of the batch, that gridding changes nothing, restarts, vehicles that are absent, the
device view, and every refusal.  No tolerance appears anywhere."""
import ctypes as C
import importlib.util
import os
from functools import lru_cache

import numpy as np
import pytest

import _grid_cases as K
import test_batch_scan_gpu as SC
import test_batch_tracks_gpu as T
import test_batch_vehicles_gpu as V
from carla_social_force_model_amd import _lib
from carla_social_force_model_amd._lib import SfmLibraryError
from carla_social_force_model_amd.batch import PTR_GRID, PTR_SCAN, SfmBatch
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.grid import CH_BORDER, CH_COUNT, CH_STATIC, CH_VEHICLE, CH_VX, grid_scene, grid_slots

pytestmark = pytest.mark.gpu

SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3
BAD_WHICH = "which must be SFM_BATCH_PTR_COMMANDS, _STATE, _ZSTATE, _EPISODES, _DONE or _SCAN"


@lru_cache(maxsize=None)
def _scenes():
    return K.mixed_batch()


def _batch(scenes, device_vehicles=False):
    b = SfmBatch(default_sfm_config(), 0.05, B=len(scenes))
    b.upload(scenes, device_vehicles=device_vehicles)
    return b


def _gridded(scenes, cells, G, frame, mask=None):
    b = _batch(scenes)
    try:
        b.set_grid(cells, G=G, mask=mask, frame=frame)
        return b.grids(), b.grid_rows()
    finally:
        b.close()


@lru_cache(maxsize=None)
def _device(G, frame, kind=None):
    return _gridded(_scenes(), K.CELLS, G, frame, K.masks(kind))


@lru_cache(maxsize=None)
def _twin(G, frame, kind=None):
    ms = K.masks(kind) or [None] * len(K.SIZES)
    return [grid_scene(sc, G, K.CELLS[s], frame=frame, mask=ms[s]) for s, sc in enumerate(_scenes())]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, f"{what}: {got.shape} against {want.shape}"
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} floats differ, first (slot, channel, cv, cu) {bad[0]}: {got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}"


# ---- 1. bitwise against the twin ------------------------------------------------------------------------------------------------

def test_the_batch_holds_every_class():
    """From the twin alone: cells with several pedestrians, velocity sums, each kind of geometry, dead rows, a tile boundary."""
    rec = np.concatenate(_twin(16, 1))
    assert (rec[:, CH_COUNT] > 1).any() and rec[:, CH_VX].any()
    for ch in (CH_BORDER, CH_STATIC, CH_VEHICLE):
        assert rec[:, ch].any(), ch
    dead = ~rec.reshape(len(rec), -1).any(axis=1)
    assert dead.sum() >= 3
    assert [K.geometry_points(sc) for sc in _scenes()[:4]] == [0, K.TILE - 1, K.TILE, K.TILE + 1]
    assert K.geometry_points(_scenes()[5]) > 3 * K.TILE and 0 in K.SIZES
    assert any((a != b).any() for a, b in zip(_twin(16, 0), _twin(16, 1)) if len(a))  # frame 1 is another record


@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("G", K.GS)
def test_device_is_bitwise_the_twin(G, frame):
    (got, rows), want = _device(G, frame), _twin(G, frame)
    assert len(got) == len(K.SIZES) and np.array_equal(rows, np.arange(sum(K.SIZES)))
    for s, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"scene {s} (N = {K.SIZES[s]}), G = {G}, frame {frame}")


# ---- 2. masks and slots ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G, frame", [(16, 1), (17, 0)])
@pytest.mark.parametrize("kind", ["agent", "all", "holes"])
def test_masked_rows_get_compact_slots(kind, G, frame):
    (got, rows), want = _device(G, frame, kind), _twin(G, frame, kind)
    so = np.concatenate([[0], np.cumsum(K.SIZES)])
    flat = np.concatenate([np.asarray(m) for m in K.masks(kind)])
    assert np.array_equal(rows, np.flatnonzero(flat))                   # the slots: the masked rows, ascending over the batch
    assert np.array_equal(rows, grid_slots(K.masks(kind), so)[0])
    for s, (g, w) in enumerate(zip(got, want)):
        assert len(g) == int(K.masks(kind)[s].sum())
        _same(g, w, f"{kind}: scene {s} (N = {K.SIZES[s]}), G = {G}, frame {frame}")
    if kind == "holes":
        assert len(got[3]) == 0                                         # the 64-row scene has no gridded row
    if kind == "all":                                                   # every row spelled out is the record of mask=None
        for g, w in zip(got, _device(G, frame)[0]):
            assert np.array_equal(_bits(g), _bits(w))


def test_every_slot_is_written_whole_and_nothing_else():
    """The buffer pre-filled through the tensor view: after grid() every slot -- the zeros of a gridded row that is not live
    included -- holds the twin's record, so no float of a slot is left over and no row without a slot has written one."""
    import torch
    scenes, G = _scenes(), 15
    ms = K.masks("holes")
    ms[2] = ms[2].copy()
    ms[2][5] = True                                                     # the ghost of the 63-row scene is gridded
    b = _batch(scenes)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        b.set_grid(K.CELLS, G=G, mask=ms, frame=1)
        t = b.grid_tensor()
        assert t.shape == (len(b.grid_rows()), 6, G, G) and not t.any().item()        # zero-filled before the first grid()
        t.fill_(7.5)
        b.grid()
        seen = t.cpu().numpy()
        want = np.concatenate([grid_scene(sc, G, K.CELLS[s], frame=1, mask=ms[s]) for s, sc in enumerate(scenes)])
        _same(seen, want, "the pre-filled buffer")
        ghost = int(np.flatnonzero(b.grid_rows() == sum(K.SIZES[:2]) + 5)[0])
        assert not seen[ghost].any()
    finally:
        b.close()


@pytest.mark.parametrize("G", sorted(K.WAVE_CELLS))
def test_one_source_per_owning_wave_lands_in_its_cell(G):
    """The accumulation passes over an entry in every wave but the one that holds the cell's owning lane: sources in the first and
    the last cell of every wave and quarter (G = 32), an order triple in one cell of each wave, and a grid whose cells all belong
    to wave 0 (G = 8).  The buffer holds NaN before the launch; the device is the twin bit for bit in both frames."""
    import torch
    sc, expected = K.wave_scene(G)
    mask = [np.arange(len(sc["loc"])) == 0]
    for frame in (0, 1):
        b = _batch([sc])
        try:
            b.set_stream(torch.cuda.current_stream().cuda_stream)
            b.set_grid(1.0, G=G, mask=mask, frame=frame)
            t = b.grid_tensor()
            assert t.shape == (1, 6, G, G)
            t.fill_(float("nan"))
            b.grid()
            seen = t.cpu().numpy()
        finally:
            b.close()
        _same(seen, grid_scene(sc, G, 1.0, frame=frame, mask=mask[0]), f"G = {G}, frame {frame}")
        flat = seen[0, :3].reshape(3, -1)
        assert sorted(np.flatnonzero(flat[0]).tolist()) == sorted(expected)
        for c, v in expected.items():
            assert tuple(flat[:, c]) == v, (G, frame, c)


# ---- 3. independence ------------------------------------------------------------------------------------------------------------

def test_a_scene_does_not_depend_on_the_rest_of_the_batch():
    scenes, G = _scenes(), 17
    mixed, _ = _device(G, 1)
    for s in (5, 6, 2):                                                 # several tiles of geometry; vehicles; exactly one tile
        alone, _ = _gridded([scenes[s]], [K.CELLS[s]], G, 1)
        assert np.array_equal(_bits(alone[0]), _bits(mixed[s])), f"scene {s} alone"
    order = [6, 4, 0, 5, 2, 3]
    moved, _ = _gridded([scenes[q] for q in order], [K.CELLS[q] for q in order], G, 1)
    for pos, s in enumerate(order):
        assert np.array_equal(_bits(moved[pos]), _bits(mixed[s])), f"scene {s} at position {pos} of another batch"


# ---- 4. gridding changes nothing ------------------------------------------------------------------------------------------------

def test_gridding_changes_nothing():
    a, b = SC._modes_batch(), SC._modes_batch()
    try:
        a.set_grid(0.5, G=16, frame=1)
        a.run(3)
        before = SC._all(a)
        a.grid()
        first = a.grids()
        SC._assert_all(SC._all(a), before, "state, waypoints, modes, clocks, vehicles around grid()")
        a.run(5)
        a.grid()
        a.run(5)
        b.run(13)
        SC._assert_all(SC._all(a), SC._all(b), "run(3), grid, run(5), grid, run(5) against run(13)")
        assert any((x != y).any() for x, y in zip(first, a.grids()) if len(x))
    finally:
        a.close()
        b.close()


# ---- 5. restarts ----------------------------------------------------------------------------------------------------------------

def _check_now(b, scenes, cells, G, frame, masks, what):
    got, veh = b.grids(), b.dynamic_obstacles()
    for s, ((loc, vel), (wp, _)) in enumerate(zip(b.state(), b.waypoints())):
        _same(got[s], grid_scene(scenes[s], G, cells[s], frame=frame, mask=masks[s], state=(loc, vel), vehicles=veh[s], waypoints=wp),
              f"{what}: scene {s}")
    return got


def test_the_grid_follows_restarts_and_keeps_the_snapshot():
    import torch
    sizes = (30, 65, 0, 130, 17)
    scenes = [K.crowd(n, 6300 + q) for q, n in enumerate(sizes)]
    cells, G = (0.5, 0.75, 1.0, 0.5, 1.0), 16
    masks = K.masks("holes", sizes)
    b = _batch(scenes)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        b.run(3)
        b.snapshot()
        b.set_grid(cells, G=G, mask=masks, frame=1)                     # keeps the snapshot
        assert b.has_snapshot
        at_snapshot = _check_now(b, scenes, cells, G, 1, masks, "at the snapshot")
        b.run(20)
        moved = _check_now(b, scenes, cells, G, 1, masks, "after run(20)")
        assert any((x != y).any() for x, y in zip(at_snapshot, moved) if len(x))
        b.restart([1, 3])
        got = _check_now(b, scenes, cells, G, 1, masks, "after restart([1, 3])")
        for s in range(5):
            assert np.array_equal(_bits(got[s]), _bits((at_snapshot if s in (1, 3) else moved)[s])), f"scene {s}"
        b.run(4)
        b.restart_device(torch.as_tensor(np.array([1, 0, 0, 0, 1], np.uint8), device="cuda"))
        got = _check_now(b, scenes, cells, G, 1, masks, "after restart_device")
        for s in (0, 4):
            assert np.array_equal(_bits(got[s]), _bits(at_snapshot[s])), f"scene {s}"
        b.set_restart_noise(11, np.array([0.5, 0.5]), goal_box=np.array([1.0, 1.0]), min_gap=0.3, tries=4)
        b.restart([0, 3])
        got = _check_now(b, scenes, cells, G, 1, masks, "after a noisy restart")
        assert (got[3] != at_snapshot[3]).any() and b.restart_noise()[0].tolist() == [1, 0, 0, 1, 0]
    finally:
        b.close()


# ---- 6. vehicles as the next tick reads them ------------------------------------------------------------------------------------

def test_moving_and_absent_vehicles():
    """Device-side vehicles after run(7): the records equal the twin fed with the state and dynamic_obstacles().  Tracked vehicles
    outside their keyframes are absent (their rings at +inf): no cell counts them."""
    scenes = [V._scene(n, 6400 + q, m, slow=False) for q, (n, m) in enumerate(((64, 3), (30, 2), (0, 1), (130, 5)))]
    b = V._batch(scenes, [V._config(q, V.ALL) for q in range(4)], [0.05, 0.04, 0.05, 0.03])
    cells, G, none = (1.0, 0.75, 1.0, 1.5), 32, [None] * 4
    try:
        b.set_grid(cells, G=G)
        b.run(7)
        got = _check_now(b, scenes, cells, G, 0, none, "after run(7)")
        assert all(o[:, CH_VEHICLE].any() for o in got if len(o))
        rng = np.random.default_rng(3)
        tracks = [[T._track(rng, 3, 0, T._mid(scenes[0])), T._track(rng, 5, 0, T._mid(scenes[0])), T._track(rng, 4, 0, T._mid(scenes[0]))],
                  None, None, None]
        b.set_vehicle_tracks(tracks)
        for tau, gone in ((0, False), (4, False), (6, True)):
            while b.vehicle_tracks()[0] < tau:
                b.run(1)
            got = _check_now(b, scenes, cells, G, 0, none, f"tracked scene at tau = {tau}")
            assert got[0][:, CH_VEHICLE].any() != gone
            assert got[3][:, CH_VEHICLE].any()                          # the free vehicles of another scene are still counted
    finally:
        b.close()


# ---- 7. device view -------------------------------------------------------------------------------------------------------------

def test_device_view():
    import torch
    scenes = [K.crowd(n, 6500 + q) for q, n in enumerate((17, 0, 65))]
    b = _batch(scenes)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        b.set_grid(0.5, G=16, mask=[[3, 5], True, np.arange(65) % 2 == 0])
        assert b.grid_rows().tolist() == [3, 5] + list(range(17, 82, 2))
        ptr, nbytes = b.device_ptr(PTR_GRID)
        t = b.grid_tensor()
        assert t.shape == (35, 6, 16, 16) and t.dtype == torch.float32 and t.data_ptr() == ptr and nbytes == 35 * 6 * 256 * 4
        assert t.is_contiguous() and not t.any().item()                 # zero-filled before the first grid()
        b.run(2)
        b.grid()
        seen = t.cpu().numpy()                                          # (torch's stream: ordered behind the launch)
        assert np.array_equal(seen, np.concatenate(b.grids()))
        b.set_grid(0.5, G=17)                                           # a new buffer: the view is taken again
        assert b.grid_tensor().shape == (82, 6, 17, 17)
        b.set_grid(0.5, G=4, mask=np.zeros(82, bool))                   # grids on, nobody gridded: no buffer, an empty view
        b.grid()
        assert b.device_ptr(PTR_GRID) == (0, 0) and b.grid_tensor().shape == (0, 6, 4, 4)
        assert [g.shape for g in b.grids()] == [(0, 6, 4, 4)] * 3
    finally:
        b.close()
    e = _batch([K.crowd(0, 1)])                                         # without rows
    try:
        e.set_grid(0.5, G=8)
        e.grid()
        assert e._lib.sfm_batch_device_ptr(e._b, PTR_GRID, None) is None
        assert e.grid_tensor().shape == (0, 6, 8, 8) and e.grids()[0].shape == (0, 6, 8, 8)
    finally:
        e.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_batch_usable():
    scenes = [K.crowd(n, 6600 + q) for q, n in enumerate((17, 65))]
    L = _lib.load()
    err = lambda x: L.sfm_batch_last_error(x._b).decode()
    fp, up = _lib.fptr, _lib.u8ptr
    cell = np.float32([0.5, 0.75])
    mask = np.zeros(82, np.uint8)
    mask[::3] = 1
    M = int(mask.sum())

    def set_grid(G=8, cell=cell, mask=mask, frame=0):
        return L.sfm_batch_set_grid(b._b, G, fp(cell), up(mask), frame)

    b = SfmBatch(default_sfm_config(), 0.05, B=2)
    try:
        assert set_grid() == SFM_ERR_STATE and "sfm_batch_upload_state" in err(b)
        with pytest.raises(SfmLibraryError, match="upload"):
            b.set_grid(0.5)
        b.upload(scenes)

        def off(what):
            assert L.sfm_batch_grid(b._b) == SFM_ERR_STATE and "grids are off" in err(b), what
            out = np.zeros(M * 6 * 64, np.float32)
            assert L.sfm_batch_download_grid(b._b, fp(out)) == SFM_ERR_STATE and "grids are off" in err(b), what
            nbytes = C.c_int64(7)
            # while grids are off the value is refused exactly as an unknown `which`
            assert L.sfm_batch_device_ptr(b._b, PTR_GRID, C.byref(nbytes)) is None and nbytes.value == 0 and err(b) == BAD_WHICH, what
            assert L.sfm_batch_device_ptr(b._b, PTR_GRID + 1, C.byref(nbytes)) is None and err(b) == BAD_WHICH
            for call in (b.grid, b.grids, b.grid_tensor, b.grid_rows):
                with pytest.raises(SfmLibraryError, match="grids are off"):
                    call()

        def usable(what):
            got = b.grids()
            so = b.scene_off
            assert np.array_equal(b.grid_rows(), np.flatnonzero(mask))
            for s, (loc, vel) in enumerate(b.state()):
                _same(got[s], grid_scene(scenes[s], 8, cell[s], state=(loc, vel), mask=mask[so[s]:so[s + 1]]), f"{what}: scene {s}")
            b.run(2)

        refused = [dict(G=0), dict(G=33), dict(G=-1), dict(frame=2), dict(frame=-1)]
        refused += [dict(cell=np.float32([0.5, bad])) for bad in (0.0, -0.5, np.nan, np.inf, 2.0e6)]
        off("before set_grid")
        for kw in refused:
            assert set_grid(**kw) == SFM_ERR_INVALID, kw
        assert "scene 1: cell must be finite, > 0 and <= 1e6 metres" in err(b)
        assert set_grid(G=33) == SFM_ERR_INVALID and "G must be 1 .. 32 cells per side, got 33" in err(b)
        assert set_grid(frame=2) == SFM_ERR_INVALID and "frame must be 0 (world axes) or 1" in err(b)
        off("after refused calls on a batch without grids")
        for bad in (dict(G=0), dict(G=33), dict(G=2.5), dict(frame=2), dict(mask=np.ones(5, bool))):
            with pytest.raises(ValueError):
                b.set_grid(0.5, **bad)
        for bad in (0.0, -1.0, np.nan, np.inf, [0.5, 0.5, 0.5]):
            with pytest.raises(ValueError):
                b.set_grid(bad)
        b.run(2)
        good = lambda: b.set_grid(cell, G=8, mask=mask != 0)
        good()
        usable("first settings")
        for kw in refused:
            assert set_grid(**kw) == SFM_ERR_INVALID, kw
            usable(f"after the refused {sorted(kw)}")                    # nothing changed: 8 cells, frame 0, the mask, the sizes
        b.snapshot()
        good()                                                           # keeps the snapshot
        assert b.has_snapshot
        b.restart()
        b.set_scan(3.0, 0.3, R=8)                                        # another sensor's settings keep the grids
        assert b.device_ptr(PTR_SCAN)[1] == 82 * 16 * 4
        usable("after set_scan")
        b.set_grid(None)
        off("after set_grid(None)")
        b.run(1)
        good()
        usable("set again after off")
        old = b.device_ptr(PTR_GRID)
        assert old[1] == M * 6 * 64 * 4
        b.upload(scenes)                                                 # drops the settings and the old buffer
        assert b.grid_cells is None
        off("after upload")
        b.set_grid(cell, G=4, mask=mask != 0)
        assert b.device_ptr(PTR_GRID)[1] == M * 6 * 16 * 4 and b.grid_tensor().shape == (M, 6, 4, 4)
        good()
        usable("set again after upload")
    finally:
        b.close()


# ---- the example ----------------------------------------------------------------------------------------------------------------

def test_grid_loop_example_runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("batch_grid_loop", os.path.join(root, "examples", "batch_grid_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    episodes, arrivals = ex.run(B=8, steps=12, repeat=2, max_age=5, quiet=True)
    assert episodes >= 8 and 0 <= arrivals <= episodes                  # everyone runs out of time at least once
