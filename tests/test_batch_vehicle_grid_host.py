"""CPU tests of the vehicles' bird's-eye grid: the NumPy twin grid.grid_vehicles_scene on hand-placed scenes with exact expectations,
its reduction to the pedestrian grid's twin bit for bit, what its bits mean against a float64 statement (tests/_vehicle_grid_cases.py
derives the margin), the argument packers and their refusals, and that header, binding, Makefile and resource file agree."""
import os
import re

import numpy as np
import pytest

import _vehicle_grid_cases as VG
from carla_social_force_model_amd import _lib, grid as G, scan as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "carla-social-force-model_amd")
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. hand-placed scenes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", [0, 1])
def test_cell_edges_and_window_edges(frame):
    """GU = 4, GV = 2, 1 m cells, the vehicle at the origin heading +x: pu = x + 2, pv = y + 1.  A source on a cell edge belongs to
    the upper cell; pu == GU and pv == GV are outside, pu == 0 and pv == 0 inside; a tiny negative x / c rounds into cell (int)half."""
    peds = [(-2.0, -1.0),            # pu = 0, pv = 0: cell [0][0]
            (2.0, 0.0),              # pu = 4 == GU: outside
            (0.0, 1.0),              # pv = 2 == GV: outside
            (1.0, 0.0),              # on the edge between cu 2 and 3: cell [1][3]
            (-1.0e-9, -1.0e-9),      # pu = fl(-1e-9 + 2) = 2, pv = 1: cell [1][2], though floor of the exact value is [0][1]
            (np.nextafter(np.float32(2.0), np.float32(0.0)), 0.0),      # pu = fl(4 - 2^-23) = 4 (a tie, to even): outside by the rule
            (1.75, np.float32(1.0) - np.float32(2.0 ** -23))]           # pv = 2 - 2^-23, exact: the last cell, [1][3]
    sc = VG.hand(peds=peds)
    rec = G.grid_vehicles_scene(sc, 4, 2, 1.0, frame=frame)
    assert rec.shape == (1, 8, 2, 4) and rec.dtype == np.float32
    want = np.zeros((2, 4), np.float32)
    want[0, 0], want[1, 3], want[1, 2] = 1, 2, 1
    assert np.array_equal(rec[0, 0], want)
    # the geometry kinds take the same rule: the same points as a border and as a static ring
    sc = VG.hand(borders=[peds], statics=[peds])
    rec = G.grid_vehicles_scene(sc, 4, 2, 1.0, frame=frame)
    assert np.array_equal(rec[0, 3], want) and np.array_equal(rec[0, 4], want) and not rec[0, [0, 1, 2, 5, 6, 7]].any()


def test_the_centre_moves_the_window_along_the_heading():
    """centre = (2, 0) and heading +y: a pedestrian 2 m north of the vehicle's centre lands in the middle cell, in both frames; in
    frame 1 x is forward, so a pedestrian 3 m north lands one cell further along u, in frame 0 one further along v."""
    sc = VG.hand(peds=[(0.0, 2.0)], vehicles=[(0.0, 0.0)], yaw=[np.pi / 2])
    north = np.float32([[0.0, 1.0]])
    for frame in (0, 1):
        rec = G.grid_vehicles_scene(sc, 5, 5, 1.0, frame=frame, centre=(2.0, 0.0), headings=north)
        assert rec[0, 0, 2, 2] == 1 and rec[0, 0].sum() == 1
    sc = VG.hand(peds=[(0.0, 3.0)], vels=[(0.0, 1.5)], vehicles=[(0.0, 0.0)], vehicle_vel=[(0.0, 0.5)], yaw=[np.pi / 2])
    r0 = G.grid_vehicles_scene(sc, 5, 5, 1.0, frame=0, centre=(2.0, 0.0), headings=north)
    r1 = G.grid_vehicles_scene(sc, 5, 5, 1.0, frame=1, centre=(2.0, 0.0), headings=north)
    assert r0[0, 0, 3, 2] == 1 and r1[0, 0, 2, 3] == 1
    # the relative velocity (0, 1) is rotated like the position: forward in frame 1
    assert (r0[0, 1, 3, 2], r0[0, 2, 3, 2]) == (0.0, 1.0) and (r1[0, 1, 2, 3], r1[0, 2, 2, 3]) == (1.0, 0.0)
    # the example of the header: GU = 48, 0.5 m cells, centre (8, 0) -- 4 m behind to 20 m ahead
    for x, inside in ((-4.0, True), (-4.001, False), (19.99, True), (20.0, False)):
        rec = G.grid_vehicles_scene(VG.hand(peds=[(x, 0.0)]), 48, 20, 0.5, frame=1, centre=(8.0, 0.0))
        assert bool(rec[0, 0].sum()) == inside, x


def test_the_own_ring_is_never_counted():
    lone = VG.hand(peds=[(1.0, 1.0)], extent=(2.0, 1.0))
    rec = G.grid_vehicles_scene(lone, 32, 32, 0.5)
    assert rec[0, 0].sum() == 1 and not rec[0, 5:].any()                 # a lone vehicle: channels 5 - 7 are zero
    two = VG.hand(vehicles=[(0.0, 0.0), (3.0, 1.0)], vehicle_vel=[(1.0, 0.0), (0.25, -0.5)], extent=[(2.0, 1.0), (1.0, 0.5)])
    rec = G.grid_vehicles_scene(two, 32, 32, 0.5)
    rings = [len(r) for _, r in two["dynamic_obstacles"]]
    assert rec.shape[0] == 2 and rec[0, 5].sum() == rings[1] and rec[1, 5].sum() == rings[0]
    # every point of one vehicle adds the same term: the owner's velocity relative to the gridded vehicle
    assert np.array_equal(rec[0, 6], np.float32(-0.75) * rec[0, 5]) and np.array_equal(rec[0, 7], np.float32(-0.5) * rec[0, 5])
    assert np.array_equal(rec[1, 6], np.float32(0.75) * rec[1, 5]) and np.array_equal(rec[1, 7], np.float32(0.5) * rec[1, 5])
    only = G.grid_vehicles_scene(two, 32, 32, 0.5, mask=[False, True])
    assert only.shape[0] == 1 and np.array_equal(bits(only[0]), bits(rec[1]))


def test_an_absent_vehicle_reads_zeros_and_is_no_source():
    two = VG.hand(peds=[(1.0, 1.0)], vehicles=[(0.0, 0.0), (3.0, 1.0)])
    gone = [(np.array([np.inf, np.inf]), np.full_like(two["dynamic_obstacles"][1][1], np.inf)), two["dynamic_obstacles"][0]]
    for frame in (0, 1):
        rec = G.grid_vehicles_scene(two, 16, 16, 0.5, frame=frame, vehicles=gone)
        assert rec.shape[0] == 2 and not rec[0].any() and rec[1, 0].sum() == 1 and not rec[1, 5:].any()


@pytest.mark.parametrize("frame", [0, 1])
def test_the_pedestrian_sums_run_in_ascending_row_order(frame):
    want = VG.ordered(VG.ORDER_VALUES)
    assert want == 0 and VG.ordered(VG.ORDER_VALUES[::-1]) == 1          # the order is visible
    rec = G.grid_vehicles_scene(VG.order_scene_pedestrians(), 8, 8, 1.0, frame=frame)
    assert rec[0, 0, 4, 6] == 3 and rec[0, 1, 4, 6] == want and rec[0, 2, 4, 6] == 0
    rec = G.grid_vehicles_scene(VG.order_scene_pedestrians(VG.ORDER_VALUES[::-1]), 8, 8, 1.0, frame=frame)
    assert rec[0, 1, 4, 6] == 1


@pytest.mark.parametrize("frame", [0, 1])
def test_the_vehicle_sums_run_in_ascending_vehicle_and_point_order(frame):
    sc = VG.order_scene_vehicles()
    p = len(sc["dynamic_obstacles"][1][1])
    want = VG.ordered([v for v in VG.ORDER_VALUES for _ in range(p)])
    back = VG.ordered([v for v in VG.ORDER_VALUES[::-1] for _ in range(p)])
    assert want != back                                                   # the order is visible
    rec = G.grid_vehicles_scene(sc, 8, 8, 1.0, frame=frame, mask=[True, False, False, False])
    assert rec[0, 5, 4, 6] == 3 * p and rec[0, 6, 4, 6] == want and rec[0, 7, 4, 6] == 0
    rec = G.grid_vehicles_scene(VG.order_scene_vehicles(VG.ORDER_VALUES[::-1]), 8, 8, 1.0, frame=frame, mask=[True, False, False, False])
    assert rec[0, 6, 4, 6] == back


# ---- 2. reduction to the pedestrian grid ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("scene,g,centre", [(3, 16, VG.ZERO), (4, 31, VG.FORWARD), (5, 32, VG.FORWARD), (8, 17, VG.ZERO), (1, 8, VG.FORWARD)])
def test_channels_0_to_5_are_the_pedestrian_grid_of_a_probe_row(scene, g, centre, frame):
    """The scene without vehicle k and with a probe row appended last, at the fp32 origin with vehicle k's velocity: channels 0 - 5
    of vehicle k are grid.grid_scene of the probe row, bit for bit -- in frame 1 with the stored heading set to scan.heading32 of
    that velocity."""
    scenes, _, _ = VG.made()
    sc = scenes[scene]
    veh = sc["dynamic_obstacles"]
    M = len(veh)
    vv = np.asarray(sc["dynamic_vel"], dtype=np.float32).reshape(M, 2)
    hs = np.array(sc["dynamic_heading"], dtype=np.float32)
    checked = 0
    for k in range(min(M, 3)):
        if not np.isfinite(veh[k][0]).all() or not vv[k].any():
            continue
        h = hs.copy()
        if frame:
            hx, hy = S.heading32(np.float32([0]), np.float32([0]), vv[k, :1], vv[k, 1:], np.float32([0]), np.float32([0]))
            h[k] = (hx[0], hy[0])
        mine = G.grid_vehicles_scene(sc, g, g, VG.CELLS[scene], frame=frame, centre=centre, headings=h,
                                     mask=np.arange(M) == k)
        ox, oy = S.vehicle_scan_origin(veh[k][0], h[k], np.float32(centre))
        n = len(sc["loc"])
        probe = dict(sc)
        probe["loc"] = np.vstack([np.asarray(sc["loc"], dtype=np.float64).reshape(n, 3), [[ox, oy, 0.0]]])
        probe["vel"] = np.vstack([np.asarray(sc["vel"], dtype=np.float64).reshape(n, 3), [[vv[k, 0], vv[k, 1], 0.0]]])
        probe["waypoint"] = np.vstack([np.asarray(sc["waypoint"], dtype=np.float64).reshape(n, 3), [[ox, oy, 0.0]]])
        rest = [v for j, v in enumerate(veh) if j != k]
        ref = G.grid_scene(probe, g, VG.CELLS[scene], frame=frame, mask=np.arange(n + 1) == n, vehicles=rest)
        assert ref.shape == (1, 6, g, g)
        assert np.array_equal(bits(mine[0, :6]), bits(ref[0])), (k, np.flatnonzero((bits(mine[0, :6]) != bits(ref[0])).any(axis=(1, 2))))
        checked += bool(mine[0, :6].any())
    assert checked


# ---- 3. what the bits mean ------------------------------------------------------------------------------------------------------

TRUTH_CASES = [(3, 16, 16, 0, VG.ZERO), (3, 33, 8, 1, VG.FORWARD), (4, 32, 32, 1, VG.FORWARD), (5, 17, 15, 1, VG.ZERO),
               (6, 64, 16, 1, VG.FORWARD), (6, 32, 32, 0, VG.FORWARD), (7, 5, 64, 1, VG.ZERO), (8, 48, 20, 1, (8.0, 0.0)), (1, 16, 16, 1, VG.FORWARD)]


@pytest.mark.parametrize("scene,GU,GV,frame,centre", TRUTH_CASES)
def test_the_twin_against_float64(scene, GU, GV, frame, centre):
    """Outside the margin every source sits in floor's cell of the float64 statement; inside it the counts differ by at most the
    number of uncertain sources; the sums stay within sum_bound; and at most 1 % of the in-range sources lie in the margin."""
    scenes, _, _ = VG.made()
    sc, cell = scenes[scene], VG.CELLS[scene]
    assert np.nanmax(np.abs(np.where(np.abs(sc["loc"][:, :2]) < 1e12, sc["loc"][:, :2], 0.0)), initial=0.0) < 1000.0    # bounded extent
    rec = G.grid_vehicles_scene(sc, GU, GV, cell, frame=frame, centre=centre)
    cells = GU * GV
    in_range = uncertain = 0
    for k in range(len(sc["dynamic_obstacles"])):
        t = VG.truth(sc, GU, GV, cell, frame, centre, k)
        r = rec[k].reshape(8, cells).astype(np.float64)
        if t is None:
            assert not r.any()
            continue
        kinds, tp, tv = t
        for (pu, pv, margin), ch, terms in zip(kinds, (0, 3, 4, 5), (tp, None, None, tv)):
            certain, cid, inside = VG.classify(pu, pv, margin, GU, GV)
            in_range += int(inside.sum())
            unc = int((~certain).sum())
            uncertain += unc
            low = np.bincount(cid[certain & (cid >= 0)], minlength=cells)
            assert (r[ch] >= low).all() and r[ch].sum() - low.sum() <= unc, (k, ch)
            if unc == 0:
                assert np.array_equal(r[ch], low), (k, ch)
            if terms is None:
                continue
            # the sums: per cell within sum_bound of the float64 sum over the certain sources; an uncertain source may add its term
            ok = certain & (cid >= 0)
            for q, tq in enumerate(terms):
                s64 = np.bincount(cid[ok], weights=tq[ok], minlength=cells)
                s1 = np.bincount(cid[ok], weights=np.abs(terms[0][ok]) + np.abs(terms[1][ok]), minlength=cells)
                loose = np.abs(tq[~certain]).sum() if unc else 0.0
                bound = np.array([VG.sum_bound(int(kk), s) for kk, s in zip(r[ch], s1 + loose)]) + loose
                assert (np.abs(r[ch + 1 + q] - s64) <= bound).all(), (k, ch, q)
    assert in_range > 0 and uncertain <= 0.01 * in_range, (uncertain, in_range)


def test_the_batch_holds_what_the_cases_promise():
    scenes, _, _ = VG.made()
    nb, ns, rings = VG.counts(scenes[VG.CROWDED])
    assert nb + ns + sum(rings) > VG.TILE and sum(rings) - max(rings) > VG.LIST          # unstaged geometry; more than one chunk
    lo, hi = VG.own_ring(scenes[VG.STRADDLE], 0)
    assert lo < VG.TILE < hi and VG.counts(scenes[VG.STRADDLE])[0] + VG.counts(scenes[VG.STRADDLE])[1] == lo
    assert not np.isfinite(scenes[VG.ABSENT[0]]["dynamic_obstacles"][VG.ABSENT[1]][0]).any()
    assert {len(sc["loc"]) for sc in scenes} >= {0, 1, 255, 256, 257, 1024}
    assert {len(sc["dynamic_obstacles"]) for sc in scenes} >= {0, 1, 2, 9, 70}
    # the crowded scene: the window around some vehicle holds more ring points than one chunk of the list
    rec = G.grid_vehicles_scene(scenes[VG.CROWDED], 32, 32, 1.0)
    assert rec[:, 5].sum(axis=(1, 2)).max() > VG.LIST



# ---- 4. the interface -----------------------------------------------------------------------------------------------------------

def test_packers_and_refusals():
    io = [0, 2, 2, 5]
    GU, GV, c, mk, frame, mx, my = G.vehicle_grid_arrays(io, 48, 20, 0.5, 1, None, (8, 0))
    assert (GU, GV, frame, mk) == (48, 20, 1, None) and c.dtype == np.float32 and c.tolist() == [0.5] * 3
    assert (mx, my) == (8.0, 0.0) and isinstance(mx, np.float32)
    mk = G.vehicle_grid_arrays(io, 1, 1, [0.5, 1.0, 2.0], 0, [[0, 1], [], None])[3]
    assert mk.dtype == np.uint8 and mk.tolist() == [0, 1, 1, 1, 1]
    assert G.vehicle_grid_arrays(io, 64, 16, 1e6, 0, np.array([1, 0, 0, 0, 1], bool))[3].tolist() == [1, 0, 0, 0, 1]
    assert G.vehicle_grid_arrays(io, 16, 64, 1.0, 0, [True, None, False])[3].tolist() == [1, 1, 0, 0, 0]
    bad = [dict(GU=0), dict(GU=65), dict(GV=0), dict(GV=65), dict(GU=33, GV=32), dict(GU=64, GV=17), dict(GU=4.0), dict(GU=True),
           dict(frame=2), dict(frame=-1), dict(frame=1.0), dict(cell=0.0), dict(cell=-1.0), dict(cell=np.inf), dict(cell=np.nan),
           dict(cell=2.0e6), dict(cell=[1.0, 2.0]), dict(centre=(np.nan, 0)), dict(centre=(0, np.inf)), dict(centre=(2.0e6, 0)),
           dict(centre=(0, -2.0e6)), dict(centre=1.0), dict(centre=(1, 2, 3)), dict(mask=[[1], [], [1, 1, 1]]), dict(mask=[None, None]),
           dict(mask=np.ones(4, bool)), dict(mask=[None, None, "abc"])]
    for kw in bad:
        args = dict(GU=8, GV=8, cell=1.0, frame=0, mask=None, centre=(0.0, 0.0))
        args.update(kw)
        with pytest.raises(ValueError):
            G.vehicle_grid_arrays(io, **args)
    with pytest.raises(ValueError):
        G.vehicle_grid_arrays([0, 2, 1], 8, 8, 1.0)
    sc = VG.hand(peds=[(1.0, 1.0)])
    for kw in (dict(GU=0), dict(GU=33, GV=32), dict(frame=3), dict(cell=0.0), dict(centre=(np.nan, 0)), dict(mask=[1, 0]),
               dict(headings=np.zeros((2, 2))), dict(vehicle_vel=np.zeros((3, 2)))):
        args = dict(GU=8, GV=8, cell=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            G.grid_vehicles_scene(sc, **args)


def test_slot_order():
    io = [0, 2, 2, 5, 5]
    veh, cnt = G.vehicle_grid_slots(None, io)
    assert veh.tolist() == [0, 1, 2, 3, 4] and cnt.tolist() == [2, 0, 3, 0] and veh.dtype == cnt.dtype == np.int64
    veh, cnt = G.vehicle_grid_slots([[0, 1], [], [1, 0, 1], None], io)
    assert veh.tolist() == [1, 2, 4] and cnt.tolist() == [1, 0, 2, 0]
    veh, cnt = G.vehicle_grid_slots(np.zeros(5, bool), io)
    assert veh.tolist() == [] and cnt.tolist() == [0, 0, 0, 0]
    # the twin's slots are the masked vehicles in ascending order
    sc = VG.hand(vehicles=[(0.0, 0.0), (3.0, 0.0), (0.0, 3.0)])
    full = G.grid_vehicles_scene(sc, 16, 16, 0.5)
    part = G.grid_vehicles_scene(sc, 16, 16, 0.5, mask=[True, False, True])
    assert part.shape[0] == 2 and np.array_equal(bits(part), bits(full[[0, 2]]))
    assert G.grid_vehicles_scene(sc, 16, 16, 0.5, mask=[False] * 3).shape == (0, 8, 16, 16)
    assert G.grid_vehicles_scene(VG.hand(vehicles=[]), 3, 5, 0.5).shape == (0, 8, 5, 3)


NAMES = ("sfm_batch_set_vehicle_grid", "sfm_batch_grid_vehicles", "sfm_batch_download_vehicle_grid")


def test_header_and_binding_agree():
    with open(os.path.join(ROOT, "include", "sfm_hip.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, argc in zip(NAMES, (8, 1, 2)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == argc == len(_lib.SYMBOLS[name][1]), name
        assert _lib.SINCE[name] == 17 and name in _lib.UNBUMPED
    assert _lib.ABI_VERSION == 17 and re.search(r"#define\s+SFM_ABI_VERSION\s+17\b", code)
    defs = dict(re.findall(r"#define\s+(SFM_BATCH_\w+)\s+(\d+)\s*$", code, flags=re.M))
    assert defs["SFM_BATCH_PTR_VEHICLE_GRID"] == "15" and defs["SFM_BATCH_VEHICLE_GRID_CHANNELS"] == "8"
    assert defs["SFM_BATCH_MAX_VEHICLE_GRID_SIDE"] == "64"
    from carla_social_force_model_amd import batch
    assert batch.PTR_VEHICLE_GRID == 15 and G.VEHICLE_GRID_CHANNELS == 8 and G.MAX_VEHICLE_GRID_SIDE == 64 and G.MAX_VEHICLE_GRID_CELLS == 1024
    ptrs = [int(v) for k, v in defs.items() if k.startswith("SFM_BATCH_PTR_")]
    assert len(ptrs) == len(set(ptrs))                                    # no two buffers share a value
    for name in ("set_vehicle_grid", "grid_vehicles", "vehicle_grids", "vehicle_grid_items", "vehicle_grid_tensor"):
        assert callable(getattr(batch.SfmBatch, name)), name


def test_the_build_lists_the_kernel():
    with open(os.path.join(PKG, "csrc", "Makefile")) as f:
        mk = f.read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, flags=re.M).group(1).split()
    asm = re.search(r"^asm:(.*)$", mk, flags=re.M).group(1).split()
    clean = re.search(r"^clean:\n\t(.*)$", mk, flags=re.M).group(1).split()
    assert "sfm_batch_vehicle_grid.hip" in src and "sfm_batch_vehicle_grid.hip" in asm and "sfm_batch_vehicle_grid.s" in clean
    assert "-o sfm_batch_vehicle_grid.s sfm_batch_vehicle_grid.hip" in mk
    with open(os.path.join(PKG, "csrc", "resource_usage.txt")) as f:
        lines = f.read().splitlines()
    at = [i for i, l in enumerate(lines) if "Function Name:" in l and "sfm_batch_vehicle_grid_kernel" in l]
    assert len(at) == 1
    block = "\n".join(lines[at[0]:at[0] + 14])
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", block) and re.search(r"VGPRs Spill: 0\b", block)
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", block).group(1))
    assert 0 < lds <= 80 * 1024                                           # two workgroups share a CU
    with open(os.path.join(PKG, "csrc", "sfm_batch_vehicle_grid.hip")) as f:
        kernel = f.read()
    assert "fp contract(off)" in kernel and "static_assert(sizeof(VehicleGridShared) <= 80 * 1024" in kernel
    assert not re.search(r"atomicAdd\(\s*\(?\s*float|unsafeAtomicAdd", kernel)                 # no float atomics


def test_the_example_is_importable():
    import importlib.util
    spec = importlib.util.spec_from_file_location("batch_av_grid_loop", os.path.join(ROOT, "examples", "batch_av_grid_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.run)
    with open(os.path.join(ROOT, "tools", "README.md")) as f:
        assert "batch_vehicle_grid.py" in f.read()
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_vehicle_grid.py"))
