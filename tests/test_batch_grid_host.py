"""CPU tests of the occupancy grids' host side: the twin ``grid.grid_scene`` on designed cases whose outcome is stated here, what
its bits mean against a float64 evaluation (tests/_grid_cases.py derives the margin), the argument checks, and the ABI's entry
points.  No GPU and no library needed."""
import importlib.util
import os
import re

import numpy as np
import pytest

import _grid_cases as K
from carla_social_force_model_amd import _lib, batch, grid
from carla_social_force_model_amd.grid import CH_BORDER, CH_COUNT, CH_STATIC, CH_VEHICLE, CH_VX, CH_VY, grid_arrays, grid_scene, grid_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(rec, ch=CH_COUNT):
    """{(cv, cu): count} of the nonzero cells of one row's channel."""
    return {(int(v), int(u)): float(rec[ch, v, u]) for v, u in np.argwhere(rec[ch] != 0)}


# ---- designed cases: the outcome is stated ----------------------------------------------------------------------------------------

def test_edges_of_cells_and_of_the_grid():
    """G = 4, c = 0.5: half = 2, the grid spans [-1, 1).  A source exactly on a cell edge belongs to the upper cell; pu == G is
    outside, pu == 0 inside; -0.0 is 0."""
    sc = K.tiny([[0, 0], [0.5, 0], [1.0, 0], [-1.0, 0], [-0.0, -0.0], [0, 1.0], [0, -1.0]])
    rec = grid_scene(sc, 4, 0.5, mask=np.arange(7) == 0)
    assert rec.shape == (1, 6, 4, 4) and rec.dtype == np.float32
    # (0.5, 0): pu = 3; (1, 0): pu = 4, outside; (-1, 0): pu = 0; (-0, -0): the centre, cell [2][2]; (0, 1) outside; (0, -1): pv = 0
    assert _counts(rec[0]) == {(2, 3): 1.0, (2, 0): 1.0, (2, 2): 1.0, (0, 2): 1.0}
    assert not rec[0, 1:].any()


def test_a_tiny_negative_offset_rounds_up_into_the_next_cell():
    """G = 16, c = 0.5: half = 8.  fx = -2^-30 gives fx / c = -2^-29 and pu = fl(8 - 2^-29) = 8: the RULE puts the source in cell 8,
    where float64 says 7.  fx = 4 - 2^-22 gives pu = fl(16 - 2^-21) = 16 (the tie goes to even): outside, where float64 says 15."""
    sc = K.tiny([[0, 0], [-2.0 ** -30, 0], [4 - 2.0 ** -22, 0], [0, -2.0 ** -30]])
    rec = grid_scene(sc, 16, 0.5, mask=np.arange(4) == 0)
    assert _counts(rec[0]) == {(8, 8): 2.0}
    pu, pv = K.truth(sc, 16, 0.5, 0, 0)[0][0]
    assert np.floor(pu).tolist() == [7.0, 15.0, 8.0] and np.floor(pv).tolist() == [8.0, 8.0, 7.0]


@pytest.mark.parametrize("G", [3, 4, 1])
def test_odd_even_and_one_cell(G):
    """c = 1.  G = 3: half = 1.5, the row's own place is the middle of cell 1.  G = 4: half = 2, it is the corner of cells 1 and 2
    and belongs to 2.  G = 1: one cell, [-0.5, 0.5)."""
    h = G / 2.0
    sc = K.tiny([[0, 0], [0, 0], [-h, -h], [h, 0], [0, h], [0.25, -0.5]])
    rec = grid_scene(sc, G, 1.0, mask=np.arange(6) == 0)
    mid = G // 2                                                       # (int)(0 / 1 + G / 2)
    want = {}
    # the coincident row; the lower corner; (0.25, -0.5); (h, 0) and (0, h) are outside
    for cell in ((mid, mid), (0, 0), (int(-0.5 + h), int(0.25 + h))):
        want[cell] = want.get(cell, 0.0) + 1.0
    assert _counts(rec[0]) == want
    assert rec[0, CH_COUNT].sum() == 3


def test_a_row_alone_sees_nothing_and_itself_is_not_counted():
    for frame in (0, 1):
        rec = grid_scene(K.tiny([[3, 4]], vel=[[1, 0]]), 5, 0.5, frame=frame)
        assert rec.shape == (1, 6, 5, 5) and not rec.any()
    rec = grid_scene(K.tiny([[3, 4], [3.25, 4]]), 5, 0.5)
    assert rec[:, CH_COUNT].sum() == 2 and rec[0, CH_COUNT, 2, 3] == 1 and rec[1, CH_COUNT, 2, 2] == 1   # each sees the other only


def test_dead_rows_as_source_and_as_gridded_row():
    """A ghost parked far away and a NaN position: neither is a source, and gridded they read zeros."""
    sc = K.tiny([[0, 0], [4.0e12, 0.25], [np.nan, 0], [0.25, 0.25], [0.25, np.nan]],
                borders=[[[0.25, 0.25]]])
    rec = grid_scene(sc, 4, 0.5)
    assert rec.shape == (5, 6, 4, 4)
    assert _counts(rec[0]) == {(2, 2): 1.0} and _counts(rec[0], CH_BORDER) == {(2, 2): 1.0}
    assert _counts(rec[3]) == {(1, 1): 1.0}
    assert not rec[[1, 2, 4]].any()
    assert grid_scene(sc, 4, 0.5, mask=[False, True, False, True, False]).shape == (2, 6, 4, 4)


def test_absent_vehicles_and_nan_points_are_never_binned():
    ring = np.full((6, 2), np.inf)
    sc = K.tiny([[0, 0], [0.5, 0.5]], vehicles=[ring, [[0.25, 0], [np.nan, 0], [0, -np.inf]]], statics=[[[-0.25, 0]]])
    for frame in (0, 1):
        rec = grid_scene(sc, 4, 0.5, frame=frame)
        assert rec[:, CH_VEHICLE].sum() == 2 and rec[:, CH_STATIC].sum() == 2 and np.isfinite(rec).all()


def test_channels_of_geometry():
    """Borders are channel 3, static obstacles 4, vehicles 5."""
    sc = K.tiny([[0, 0]], borders=[[[0.25, 0.25], [0.3125, 0.25]], [[-0.75, 0]]], statics=[[[0.75, -0.75]]],
                vehicles=[[[-0.75, -0.75], [-0.75, -0.75], [-0.75, -0.625]]])
    rec = grid_scene(sc, 4, 0.5)[0]
    assert _counts(rec, CH_BORDER) == {(2, 2): 2.0, (2, 0): 1.0}
    assert _counts(rec, CH_STATIC) == {(0, 3): 1.0}
    assert _counts(rec, CH_VEHICLE) == {(0, 0): 3.0}
    assert not rec[:3].any()


def test_heading_frame():
    """Frame 1, G = 4, c = 0.5.  Row 0 stands still and heads for its goal straight up (+y): forward is +y, left is -x.  Row 1 walks
    along -x.  Row 2 has neither a velocity nor a way to go: heading (1, 0), the world's axes."""
    sc = K.tiny([[0, 0], [0, 0.5], [-0.5, 0]], vel=[[0, 0], [-1, 0], [0, 0]], waypoint=[[0, 5], [0, 0.5], [-0.5, 0]])
    rec = grid_scene(sc, 4, 0.5, frame=1)
    # row 0: (0, 0.5) is 0.5 ahead: pu = 3, pv = 2; (-0.5, 0) is 0.5 to the left: pu = 2, pv = 3
    assert _counts(rec[0]) == {(2, 3): 1.0, (3, 2): 1.0}
    # ... row 1's velocity (-1, 0) is 1 to the left: (fx, fy) = (0, 1)
    assert rec[0, CH_VX, 2, 3] == 0.0 and rec[0, CH_VY, 2, 3] == 1.0
    # row 1 heads along -x: row 0 at (0, -0.5) relative is 0.5 to its left, row 2 at (-0.5, -0.5) is 0.5 ahead and 0.5 left
    assert _counts(rec[1]) == {(3, 2): 1.0, (3, 3): 1.0}
    assert rec[1, CH_VX, 3, 2] == -1.0 and rec[1, CH_VY, 3, 2] == 0.0   # row 0 stands: relative (1, 0) in the world, -1 forward
    # row 2: heading (1, 0), the record of frame 0
    assert np.array_equal(rec[2], grid_scene(sc, 4, 0.5, frame=0)[2])
    assert _counts(rec[2]) == {(2, 3): 1.0, (3, 3): 1.0}


def test_velocity_sums_are_formed_in_ascending_order():
    """Three sources in one cell with relative velocities 1, 1e8, -1e8 along x, in row order: ascending, fp32 gives (1 + 1e8) - 1e8
    = 0; descending it would give (-1e8 + 1e8) + 1 = 1.  Along y the same with the roles swapped."""
    sc = K.tiny([[0, 0], [0.125, 0], [0.25, 0], [0.375, 0]], vel=[[0, 0], [1, -1.0e8], [1.0e8, 1.0e8], [-1.0e8, 1]])
    rec = grid_scene(sc, 4, 0.5, mask=np.arange(4) == 0)[0]
    assert rec[CH_COUNT, 2, 2] == 3
    assert rec[CH_VX, 2, 2] == 0.0 and rec[CH_VY, 2, 2] == 1.0
    one, big = np.float32(1), np.float32(1.0e8)
    assert (np.float32(0) + -big + big) + one == 1.0 and (np.float32(0) + one + big) + -big == 0.0   # the other order, other bits
    # a sum, not a mean
    sc = K.tiny([[0, 0], [0.125, 0], [0.25, 0]], vel=[[0.5, 0], [1, 2], [1, 2]])
    rec = grid_scene(sc, 4, 0.5, mask=np.arange(3) == 0)[0]
    assert rec[CH_VX, 2, 2] == 1.0 and rec[CH_VY, 2, 2] == 4.0 and rec[CH_COUNT, 2, 2] == 2


@pytest.mark.parametrize("G", sorted(K.WAVE_CELLS))
def test_one_source_per_owning_wave_lands_in_its_cell(G):
    """The scene of the device's wave test, from the twin alone: the cells and the sums are the ones stated by hand, in both
    frames, and the order triple sums to 0 -- which no other order of the three adds gives."""
    sc, expected = K.wave_scene(G)
    hit, triple = K.WAVE_CELLS[G]
    if G == 32:
        owners = {((c // K.WAVE) % 4, c // K.BLOCK, c % K.WAVE) for c in hit}
        assert owners == {(w, q, l) for w in range(4) for q in range(4) for l in (0, 63)}
        assert sorted((c // K.WAVE) % 4 for c in triple) == [0, 1, 2, 3]
    else:
        assert G * G <= K.WAVE                                          # waves 1 to 3 own no cell
    assert 36 <= len(sc["loc"]) <= 44 or G == 8
    mask = np.arange(len(sc["loc"])) == 0
    want = np.zeros((3, G * G), np.float32)
    for c, v in expected.items():
        want[:, c] = v
    for frame in (0, 1):
        rec = grid_scene(sc, G, 1.0, frame=frame, mask=mask)
        assert rec.shape == (1, 6, G, G) and not rec[0, CH_BORDER:].any()
        assert np.array_equal(rec[0, :3].reshape(3, -1).view(np.uint32), want.view(np.uint32)), (G, frame)
    ordered = lambda vs: np.float32(np.float32(np.float32(vs[0]) + np.float32(vs[1])) + np.float32(vs[2]))
    assert ordered(K.ORDER_VALUES) == 0.0 and ordered(K.ORDER_VALUES[1:] + K.ORDER_VALUES[:1]) == 1.0     # the order shows
    assert all(want[1, c] == 0.0 and want[0, c] == 3.0 for c in triple)


def test_cell_size_scales_before_the_shift():
    """pu = fx / c + half, not (fx + half) / c: with c = 0.25 a source 0.5 away is two cells from the centre."""
    rec = grid_scene(K.tiny([[0, 0], [0.5, -0.25]]), 6, 0.25, mask=[True, False])[0]
    assert _counts(rec) == {(2, 5): 1.0}


def test_state_vehicles_and_waypoints_are_fed_in():
    sc = K.tiny([[0, 0], [5, 5]], vehicles=[[[9, 9]]])
    rec = grid_scene(sc, 4, 0.5, frame=1, mask=[True, False], state=(np.array([[0, 0, 0], [0.5, 0, 0]]), np.zeros((2, 3))),
                     vehicles=[(np.zeros(2), np.array([[0, 0.5]]))], waypoints=np.array([[0, 3, 0], [0, 0, 0]]))[0]
    assert _counts(rec) == {(1, 2): 1.0} and _counts(rec, CH_VEHICLE) == {(2, 3): 1.0}      # heading +y: +x is to the right


# ---- what the bits mean -----------------------------------------------------------------------------------------------------------

_SCENES = K.mixed_batch()


def _sample(n):
    return np.unique(np.linspace(0, n - 1, 12).astype(np.int64)) if n else np.zeros(0, np.int64)


@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("G", K.GS)
def test_the_twin_is_floor_of_float64_away_from_cell_edges(G, frame):
    """For every source whose float64 cell coordinates lie further than delta from an integer, the twin's cell is floor of them; the
    sources inside the margin are at most 1 % of the in-range ones on every input; every velocity sum lies within the bound of
    sequential summation of its float64 sum."""
    d = K.delta(G, frame)
    seen = 0
    for s, sc in enumerate(_SCENES):
        n = len(sc["loc"])
        rows = _sample(n)
        if not len(rows):
            continue
        mask = np.zeros(n, bool)
        mask[rows] = True
        rec = grid_scene(sc, G, K.CELLS[s], frame=frame, mask=mask).reshape(len(rows), 6, G * G)
        in_range = margin = 0
        with np.errstate(all="ignore"):
            live = (np.abs(sc["loc"][:, 0]) < 1e12) & (np.abs(sc["loc"][:, 1]) < 1e12)
        for q, row in enumerate(rows):
            if not live[row]:
                assert not rec[q].any()
                continue
            kinds, (tx, ty) = K.truth(sc, G, K.CELLS[s], frame, row)
            clean = True
            for ch, (pu, pv) in zip((CH_COUNT, CH_BORDER, CH_STATIC, CH_VEHICLE), kinds):
                certain, cell = K.classify(pu, pv, G, d)
                want = np.bincount(cell[certain & (cell >= 0)], minlength=G * G)
                unsure = int((~certain).sum())
                in_range += int((cell >= 0).sum())
                margin += unsure
                clean &= unsure == 0 or ch != CH_COUNT
                diff = rec[q, ch] - want
                assert (diff >= 0).all() and diff.sum() <= unsure, f"scene {s}, row {row}, channel {ch}: {unsure} sources in the margin"
            if clean:                                                  # every pedestrian's cell is certain: the sums, cell by cell
                certain, cell = K.classify(*kinds[0], G, d)
                for c in np.unique(cell[cell >= 0]):
                    pick = cell == c
                    k, size = int(pick.sum()), float(np.hypot(tx[pick], ty[pick]).sum())
                    for ch, t in ((CH_VX, tx), (CH_VY, ty)):
                        assert abs(float(rec[q, ch, c]) - t[pick].sum()) <= K.sum_bound(k, size), f"scene {s}, row {row}, cell {c}"
        assert margin <= 0.01 * in_range, f"scene {s}: {margin} of {in_range} in-range sources lie in the margin"
        seen += in_range
    assert seen > 0


# ---- argument checks ------------------------------------------------------------------------------------------------------------

def test_grid_arrays_refusals():
    G, c, frame = grid_arrays(3, 16, 0.5, 1)
    assert G == 16 and frame == 1 and c.dtype == np.float32 and c.tolist() == [0.5] * 3
    assert grid_arrays(2, np.int64(32), [0.5, 1.0])[1].tolist() == [0.5, 1.0]
    for bad in (0, 33, -1, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match="G must be"):
            grid_arrays(2, bad, 0.5)
    for bad in (0.0, -0.5, np.nan, np.inf, 2.0e6, [0.5, 0.0], [0.5, 0.5, 0.5], "x"):
        with pytest.raises(ValueError, match="cell"):
            grid_arrays(2, 16, bad)
    for bad in (2, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="frame"):
            grid_arrays(2, 16, 0.5, bad)
    with pytest.raises(ValueError):
        grid_scene(K.tiny([[0, 0]]), 0, 0.5)
    with pytest.raises(ValueError):
        grid_scene(K.tiny([[0, 0]]), 4, 0.0)


def test_grid_slots():
    so = np.array([0, 3, 3, 5, 9], np.int32)
    rows, counts = grid_slots(None, so)
    assert rows.tolist() == list(range(9)) and counts.tolist() == [3, 0, 2, 4]
    rows, counts = grid_slots([[2], False, [0, 1], np.array([True, False, False, True])], so)
    assert rows.tolist() == [2, 3, 4, 5, 8] and counts.tolist() == [1, 0, 2, 2]
    m = np.zeros(9, bool)
    rows, counts = grid_slots(m, so)
    assert rows.shape == (0,) and counts.tolist() == [0, 0, 0, 0]
    for bad in ([[0]], np.ones(8, bool), [[3], False, [0], [0]], np.ones(9, np.float32), [[0.5], False, [0], [0]]):
        with pytest.raises(ValueError):
            grid_slots(bad, so)
    with pytest.raises(ValueError):
        grid_slots(None, np.array([0, 3, 2]))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared():
    src = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    for name, nargs in (("sfm_batch_set_grid", 5), ("sfm_batch_grid", 1), ("sfm_batch_download_grid", 2)):
        assert re.search(r"\b%s\(" % name, src), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs and _lib.SINCE[name] == 17
        assert name in _lib.UNBUMPED                                     # an older build of the same ABI number still loads
    assert re.search(r"#define SFM_ABI_VERSION 17\b", src) and _lib.ABI_VERSION == 17
    assert re.search(r"#define SFM_BATCH_PTR_GRID 7\b", src) and batch.PTR_GRID == 7
    assert re.search(r"#define SFM_BATCH_MAX_GRID 32\b", src) and grid.MAX_GRID == 32
    assert re.search(r"#define SFM_BATCH_GRID_CHANNELS 6\b", src) and grid.GRID_CHANNELS == 6
    for method in ("set_grid", "grid", "grids", "grid_rows", "grid_tensor"):
        assert callable(getattr(batch.SfmBatch, method))
    csrc = os.path.join(ROOT, "carla-social-force-model_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "sfm_batch_grid.hip" in mk.split("SRC", 1)[1].split("\n", 1)[0] and "-o sfm_batch_grid.s sfm_batch_grid.hip" in mk
    assert "sfm_batch_grid_kernel" in open(os.path.join(csrc, "resource_usage.txt")).read()


def test_the_example_imports_without_a_gpu():
    spec = importlib.util.spec_from_file_location("batch_grid_loop", os.path.join(ROOT, "examples", "batch_grid_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    assert callable(ex.run)
