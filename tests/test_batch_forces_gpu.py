"""GPU tests of the batch's force records (sfm_batch_tick_forces, sfm_batch_run_recorded_forces; SfmBatch.tick_forces /
run_recorded_forces): every force of every scene against the oracle, the total against the velocity update, recording that does
not perturb the run, frames against step-wise ticks, scene independence, masks and zeros, and refused input.
Run on the MI355X box with  python -m pytest tests/test_batch_forces_gpu.py -m gpu."""
import ctypes as C

import numpy as np
import pytest

import _parity as P
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import FORCE_RECORD_NAMES, SfmBatch
from carla_social_force_model_amd.config import default_sfm_config
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

ALL = scenarios.ALL_FORCES
DT = 1.0
MSF = 1e4
SIZES = (1, 5, 64, 100, 128, 129, 300, 1024)        # S = 4 / 2 / 1 j-slices, one pass and several
CROSSING, ROAD_TO_SIDEWALK, GONE = 2, 3, 255
SFM_ERR_STATE = -3


def _scene(n, seed, z_spread=0.0, dyn_scale=1.0, border_len=(3.0, 15.0)):
    sc = vars(scenarios.make_scenario(n, seed, n_borders=2, n_static=2, n_dynamic=4, z_spread=z_spread, border_len=border_len))
    rng = np.random.default_rng(seed + 31)
    sc["radius"] = np.float32(rng.uniform(0.2, 0.45, n)).astype(np.float64)
    sc["crossing"] = rng.random(n) < 0.2
    sc["dynamic_vel"] = np.float32(sc["dynamic_vel"] * dyn_scale).astype(np.float64)
    return sc


def _cfg(k=0, forces=ALL, msf=MSF, pow2=False):
    cfg = default_sfm_config(forces)
    cfg["max_speed_factor"] = msf
    cfg["use_ped_radius"] = bool(k % 2)
    if pow2:                                           # -A * sum exact in fp32: the fused products of the total round as the parts
        cfg["pedestrian_force"]["A"] = 4.0
        cfg["static_obstacle_force"]["A"] = 16.0
        cfg["dynamic_obstacle_force"]["A"] = 32.0
    return cfg


def _oracle(sc, cfg):
    n = len(sc["loc"])
    prm = O.OracleParams.from_config(cfg)
    geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"], sc["dynamic_obstacles"],
                      sc["dynamic_vel"])
    crossing = sc.get("crossing")
    crossing = np.zeros(n, bool) if crossing is None else crossing
    f32 = lambda a: np.float32(a).astype(np.float64)   # the state as the batch holds it
    diag = {}
    with np.errstate(all="ignore"):
        forces, total, _ = O.tick_forces(f32(sc["loc"]), f32(sc["vel"]), f32(sc["waypoint"]), f32(sc["target_speed"]),
                                         f32(sc["radius"]), crossing, geom, prm, theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
    forces["total"] = total
    return forces, diag


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b, what):
    assert a.shape == b.shape, f"{what}: shapes {a.shape} {b.shape}"
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: not bitwise equal"


# ---- 1. per-force parity with the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_tick_forces_match_the_oracle_force_by_force(z_spread):
    """Scenes of every slice split, all five forces (2 borders, 2 static obstacles, 4 vehicles, a crossing mask), radius on in
    alternate scenes; each force and the total held to check_force with the oracle's per-force exposure (argmin ties, culls and
    sign(theta) flips within fp32 noise).  The plain bound everywhere: no conditioned allowance is needed for forces, whose scale
    is the sum of their term magnitudes."""
    scenes = [_scene(n, 4100 + k, z_spread) for k, n in enumerate(SIZES)]
    cfgs = [_cfg(k) for k in range(len(SIZES))]
    b = SfmBatch(cfgs, DT)
    try:
        b.upload(scenes)
        assert b.planar == (z_spread == 0.0)
        before = b.state()
        rec = b.tick_forces(integrate=False)
        after = b.state()
    finally:
        b.close()
    Cc = 2 if z_spread == 0.0 else 3
    worst = {}
    for k, (sc, cfg, got) in enumerate(zip(scenes, cfgs, rec)):
        assert np.array_equal(before[k][0], after[k][0])     # flags = 0: v' only, nobody moved
        ref, diag = _oracle(sc, cfg)
        assert sorted(got) == sorted(FORCE_RECORD_NAMES)
        for name in FORCE_RECORD_NAMES:
            g = got[name]
            assert g.dtype == np.float32 and g.shape == (len(sc["loc"]), Cc)
            gz = np.zeros((len(g), 3))
            gz[:, :Cc] = g
            ex, ab = diag[name]
            w, _ = P.check_force(f"scene {k} N={len(g)} {name}", gz, ref[name], ab, ex)
            worst[name] = max(worst.get(name, 0.0), w)
            if name in ("border_force", "static_obstacle_force", "dynamic_obstacle_force") and Cc == 3:
                assert (g[:, 2] == 0).all()
    print("\nbatch force record " + ("planar" if Cc == 2 else "3-D") + ": worst err/scale " +
          ", ".join(f"{n} {w:.2e}" for n, w in worst.items()))


# ---- 2. the total is the velocity update's input -------------------------------------------------------------------------------
@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_total_is_the_sum_of_the_parts_and_the_velocity_input(z_spread):
    """The recorded total is (((acc + ped) + border) + static) + dynamic of the recorded parts in float32, bitwise -- with A a
    power of two (and tau = 0.5), so that the -A products the tick fuses into its additions are exact -- and, at dt = 1 with the
    cap out of reach, it is the F that moved v to v' (check_force_from_velocity).  At the stock A it is that sum to one rounding
    per product."""
    for pow2 in (True, False):
        scenes = [_scene(n, 4300 + k, z_spread) for k, n in enumerate((7, 64, 200, 1024))]
        cfgs = [_cfg(k, pow2=pow2) for k in range(len(scenes))]
        b = SfmBatch(cfgs, DT)
        try:
            b.upload(scenes)
            v_in = [v for _, v in b.state()]
            rec = b.tick_forces(integrate=True)
            v_out = [v for _, v in b.state()]
        finally:
            b.close()
        for k, got in enumerate(rec):
            parts = [got[n] for n in FORCE_RECORD_NAMES[:5]]
            s = (((parts[0] + parts[1]) + parts[2]) + parts[3]) + parts[4]
            if pow2:
                _same_bits(s, got["total"], f"scene {k}: total")
            else:
                scale = sum(np.abs(p) for p in parts)
                assert (np.abs(s - got["total"]) <= 4 * np.finfo(np.float32).eps * scale).all(), f"scene {k}"
            Cc = got["total"].shape[1]
            F = np.zeros((len(s), 3))
            F[:, :Cc] = got["total"]
            mag = np.linalg.norm(F, axis=1)
            w, _ = P.check_force_from_velocity(f"scene {k} total", v_out[k], v_in[k], DT, F, mag, np.zeros(len(s)),
                                               np.float32(scenes[k]["target_speed"]) * MSF)


# ---- 3. and 4. recording does not perturb; frame f's forces are tick f*stride's --------------------------------------------------
KINDS = ("plain", "redraw", "vehicles", "modes")


def _twin(kind, z_spread=0.0):
    scenes, plans = [], []
    for k, n in enumerate((3, 64, 150, 64)):
        sc = _scene(n, 4500 + k, z_spread, dyn_scale=0.1)
        if kind == "modes":
            plan, _ = scenarios.make_mode_plan(sc, 4600 + k)
            plans.append(plan)
        scenes.append(sc)
    b = SfmBatch([_cfg(k, msf=1.3) for k in range(len(scenes))], 0.05)
    b.upload(scenes, device_vehicles=kind in ("vehicles", "modes"))
    if kind == "redraw":
        b.set_waypoint_streams([11, 12, 13, 14], [s["world_side"] for s in scenes], 1.0)
    if kind == "modes":
        b.set_modes(plans, sim_time0=[0.0, 1.0, 2.0, 3.0], scenes=scenes)
    return b


def _everything(b, kind):
    out = [b.state(), b.waypoints()]
    if kind in ("vehicles", "modes"):
        out.append(b.dynamic_obstacles())
    if kind == "modes":
        out += [b.modes(), b.clocks()]
    return out


def _assert_tree_equal(x, y, what):
    if isinstance(x, np.ndarray):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), what
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), what
        for k, (u, v) in enumerate(zip(x, y)):
            _assert_tree_equal(u, v, f"{what}[{k}]")
    else:
        assert x == y, what


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
@pytest.mark.parametrize("kind", KINDS)
def test_recording_forces_does_not_perturb_the_run(kind, z_spread):
    ticks, stride = 23, 4
    redraw = kind == "redraw"
    a, b = _twin(kind, z_spread), _twin(kind, z_spread)
    try:
        fa, ia, za = a.run_recorded(ticks, stride, redraw=redraw)
        fb, ib, zb, rec = b.run_recorded_forces(ticks, stride, redraw=redraw)
        assert np.array_equal(ia, ib) and len(ib) == 6
        _assert_tree_equal(fa, fb, "frames")
        _assert_tree_equal(za, zb, "zframes")
        _assert_tree_equal(_everything(a, kind), _everything(b, kind), "state after the run")
        for k, d in enumerate(rec):
            n = fb[k].shape[1]
            for name in FORCE_RECORD_NAMES:
                assert d[name].shape == (6, n, 2 if z_spread == 0.0 else 3), (k, name)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_frame_forces_are_the_forces_of_that_tick(kind):
    ticks, stride = 14, 3
    redraw = kind == "redraw"
    a, b = _twin(kind), _twin(kind)
    try:
        frames, _, _, rec = a.run_recorded_forces(ticks, stride, redraw=redraw, forces=("pedestrian_force", "border_force", "total"))
        f = 0
        for t in range(ticks):
            if t % stride == 0:
                got = b.tick_forces(integrate=True, redraw=redraw, forces=("pedestrian_force", "border_force", "total"))
                for k, d in enumerate(got):
                    assert sorted(d) == sorted(rec[k])
                    for name in d:
                        _same_bits(rec[k][name][f], d[name], f"tick {t} scene {k} {name}")
                f += 1
            else:
                b.tick(integrate=True, redraw=redraw)
        assert f == len(frames[0])
        _assert_tree_equal(_everything(a, kind), _everything(b, kind), "state after the run")
    finally:
        a.close()
        b.close()


# ---- 5. scene independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_a_scenes_record_does_not_depend_on_the_batch(z_spread):
    probe = _scene(100, 4700, z_spread)
    others = [_scene(n, 4710 + k, z_spread) for k, n in enumerate((1, 64, 300, 1024, 7))]
    cfg = _cfg(1)
    alone = SfmBatch(cfg, DT, B=1)
    try:
        alone.upload([probe], planar=z_spread == 0.0)
        ref = alone.tick_forces()[0]
    finally:
        alone.close()
    for pos in (0, 3, 5):
        scenes = others[:pos] + [probe] + others[pos:]
        b = SfmBatch([_cfg(k) if k != pos else cfg for k in range(len(scenes))], DT)
        try:
            b.upload(scenes, planar=z_spread == 0.0)
            got = b.tick_forces()[pos]
        finally:
            b.close()
        for name in FORCE_RECORD_NAMES:
            _same_bits(got[name], ref[name], f"position {pos}: {name}")


# ---- 6. masks and zeros -------------------------------------------------------------------------------------------------------
def test_subset_masks_are_slices_of_the_full_record():
    scenes = [_scene(n, 4800 + k) for k, n in enumerate((5, 64, 200))]
    cfgs = [_cfg(k) for k in range(3)]
    full = None
    for sel in (None, ("total",), ("acceleration_force", "dynamic_obstacle_force"), ("border_force", "pedestrian_force", "total")):
        b = SfmBatch(cfgs, DT)
        try:
            b.upload(scenes)
            got = b.tick_forces(forces=sel)
        finally:
            b.close()
        if full is None:
            full = got
            continue
        for k, d in enumerate(got):
            assert list(d) == [n for n in FORCE_RECORD_NAMES if n in sel]
            for name in d:
                _same_bits(d[name], full[k][name], f"{sel}: scene {k} {name}")


def test_a_force_switched_off_records_zeros_beside_a_scene_that_has_it():
    scenes = [_scene(64, 4900 + k, border_len=(20.0, 40.0)) for k in range(6)]
    cfgs = [_cfg(0, forces=[f for f in ALL if f != ALL[k % 5]]) if k < 5 else _cfg(0) for k in range(6)]
    b = SfmBatch(cfgs, DT)
    try:
        b.upload(scenes)
        got = b.tick_forces()
    finally:
        b.close()
    for k in range(5):
        off = ALL[k]
        assert (got[k][off] == 0).all(), f"scene {k}: {off} is off"
        assert (np.abs(got[5][off]).sum() > 0), f"scene 5 has {off}"
        for name in ALL:
            if name != off:
                assert np.abs(got[k][name]).sum() > 0, f"scene {k}: {name} is on"


def test_modes_zero_the_border_force_on_the_road_and_every_force_of_a_despawned_row():
    b = _twin("modes")
    try:
        seen_road = seen_gone = 0
        for t in range(160):
            before = [m.copy() for m, _, _ in b.modes()]
            got = b.tick_forces(integrate=True)
            after = [m for m, _, _ in b.modes()]
            for k, d in enumerate(got):
                road = np.isin(before[k], (CROSSING, ROAD_TO_SIDEWALK)) & np.isin(after[k], (CROSSING, ROAD_TO_SIDEWALK))
                assert (d["border_force"][road] == 0).all(), f"tick {t} scene {k}"
                gone = before[k] == GONE
                for name in FORCE_RECORD_NAMES:
                    assert (d[name][gone] == 0).all(), f"tick {t} scene {k} {name} of a despawned row"
                seen_road += int(road.sum())
                seen_gone += int(gone.sum())
        assert seen_road > 0 and seen_gone > 0, (seen_road, seen_gone)
    finally:
        b.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_usable():
    L = _lib.load()
    params = (_lib.SfmParamsC * 2)()
    from carla_social_force_model_amd.engine import params_from_config
    for k in range(2):
        params[k] = params_from_config(_cfg(0), 0.05)          # (no radii: use_ped_radius off)
    h = C.c_void_p()
    assert L.sfm_batch_create(2, params, 0, C.byref(h)) == 0
    try:
        err = lambda: L.sfm_batch_last_error(h).decode()
        buf = np.zeros(4 * 6 * 8 * 2, np.float32)                      # 4 frames of six planar forces of 8 rows
        frames = np.zeros(4 * 8 * 4, np.float32)
        got = C.c_int(-1)
        assert L.sfm_batch_tick_forces(h, 0, 0x3F, buf.ctypes.data) == SFM_ERR_STATE and "upload" in err()    # no state yet
        assert L.sfm_batch_run_recorded_forces(h, 4, 0, 1, 0x3F, frames.ctypes.data, None, buf.ctypes.data, 4,
                                               C.byref(got)) == SFM_ERR_STATE and "upload" in err()
        rng = np.random.default_rng(3)
        so = np.array([0, 5, 8], np.int32)
        cols = {c: np.float32(rng.uniform(0, 5, 8)) for c in ("x", "y", "vx", "vy", "wx", "wy", "target_speed")}
        f = lambda c: cols[c].ctypes.data
        assert L.sfm_batch_upload_state(h, so.ctypes.data, f("x"), f("y"), None, f("vx"), f("vy"), None, f("wx"), f("wy"),
                                        f("target_speed"), None, None) == 0
        state = lambda: [np.array(v) for v in _download(L, h, 8)]
        s0 = state()
        for mask in (0, 1 << 6, 0x7F):
            assert L.sfm_batch_tick_forces(h, 0, mask, buf.ctypes.data) != 0 and "force_mask" in err()
            assert L.sfm_batch_run_recorded_forces(h, 4, 0, 1, mask, frames.ctypes.data, None, buf.ctypes.data, 4,
                                                   C.byref(got)) != 0 and "force_mask" in err()
        assert L.sfm_batch_tick_forces(h, 0, 0x3F, None) != 0 and "NULL" in err()
        assert L.sfm_batch_run_recorded_forces(h, 4, 0, 1, 0x3F, frames.ctypes.data, None, None, 4, C.byref(got)) != 0 and "NULL" in err()
        assert L.sfm_batch_run_recorded_forces(h, 4, 0, 1, 0x3F, None, None, buf.ctypes.data, 4, C.byref(got)) != 0 and "NULL" in err()
        assert L.sfm_batch_run_recorded_forces(h, 4, 0, 1, 0x3F, frames.ctypes.data, frames.ctypes.data, buf.ctypes.data, 4,
                                               C.byref(got)) != 0 and "planar" in err()
        # frames alone fit (3e6 frames x 8 rows x 16 B = 384 MB); with all six planar forces (+ 48 B a row) they do not
        big = 3_000_000
        assert L.sfm_batch_run_recorded_forces(h, big, 0, 1, 0x3F, frames.ctypes.data, None, buf.ctypes.data, big,
                                               C.byref(got)) != 0 and "bytes" in err() and got.value == 0
        assert L.sfm_batch_tick_forces(h, _lib.TICK_REDRAW_WAYPOINTS, 0x3F, buf.ctypes.data) != 0 and "SFM_TICK_INTEGRATE" in err()
        # SFM_TICK_RECORD_FORCES stays refused by the three older entry points
        assert L.sfm_batch_tick(h, _lib.TICK_RECORD_FORCES) != 0
        assert L.sfm_batch_run(h, 2, _lib.TICK_RECORD_FORCES) != 0
        assert L.sfm_batch_run_recorded(h, 2, _lib.TICK_RECORD_FORCES, 1, frames.ctypes.data, None, 2, C.byref(got)) != 0
        for u, v in zip(s0, state()):
            assert np.array_equal(u, v)                                  # nothing was launched
        # the next valid calls work
        assert L.sfm_batch_tick_forces(h, 0, 1 << 5, buf.ctypes.data) == 0
        assert np.isfinite(buf[:16]).all()
        assert L.sfm_batch_run_recorded_forces(h, 4, 0, 2, 0x3F, frames.ctypes.data, None, buf.ctypes.data, 2,
                                               C.byref(got)) == 0 and got.value == 2
    finally:
        L.sfm_batch_destroy(h)
    # ... and through SfmBatch: SfmLibraryError
    b = SfmBatch(_cfg(0), 0.05, B=1)
    try:
        with pytest.raises(_lib.SfmLibraryError):
            b.tick_forces()                                              # nothing uploaded
        sc = _scene(9, 4990)
        b.upload([sc])
        with pytest.raises(_lib.SfmLibraryError, match="SFM_TICK_INTEGRATE"):
            b.tick_forces(redraw=True)                                   # no streams set
        with pytest.raises(_lib.SfmLibraryError, match="bytes"):
            b.run_recorded_forces(30_000_000, max_frames=30_000_000, forces="total")
        with pytest.raises(ValueError):
            b.tick_forces(forces=("no_such_force",))
        got = b.tick_forces(forces="total")
        assert list(got[0]) == ["total"] and np.isfinite(got[0]["total"]).all()
    finally:
        b.close()


def _download(L, h, n):
    cols = [np.zeros(n, np.float32) for _ in range(4)]
    assert L.sfm_batch_download_state(h, cols[0].ctypes.data, cols[1].ctypes.data, None, cols[2].ctypes.data,
                                      cols[3].ctypes.data, None) == 0
    return cols
