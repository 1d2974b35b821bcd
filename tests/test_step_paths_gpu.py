"""GPU tests of the host-in-the-loop step (SfmEngine.step_packed / step_records -> sfm_step_packed / sfm_step_records), the path a
CARLA loop takes through PedestrianSimulation.tick: v' against the C oracle across the tick planner's thresholds (ordered kernel below
256 pedestrians, symmetric pair kernel + epilogue from 256, spatial re-pack from 2048, tile-pair list above 4096), one engine through a
CARLA-like sequence of crowd sizes, vehicle counts and caller buffers, the facade through the same thresholds, and the record layouts
sfm_step_records accepts.  The step path re-uploads the state every call, writes v' through a pinned host block
(TickArgs::host_pk / host_zv) and scatters it back to the caller's order through the upload's permutation."""
import numpy as np
import pytest

import _parity as P
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd._lib import SfmLibraryError
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.engine import SfmEngine
from carla_social_force_model_amd.host_state import BORDER_FREE_MODES, PED_STATE_DTYPE, PedMode, PedModeManager
from carla_social_force_model_amd.pedestrian_simulation import PedestrianSimulation
from oracle import c_oracle
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

DT = 0.05
SIZES = [1, 2, 63, 64, 65, 511, 2047, 2048, 2049, 4096, 4097, 9000]
FULL = {2, 65, 2049, 4097, 9000}          # all five forces, vehicles, use_ped_radius, border-force-off rows
PED_ONLY = ("acceleration_force", "pedestrian_force")


def _r32(a):
    return np.asarray(np.float32(a), dtype=np.float64)


def _vehicles(M, seed, side, extent=(2.4, 1.0)):
    """M vehicles as the simulator reports them: fp32 centres, rings (ring length grows with ``extent``), velocities."""
    rng = np.random.default_rng(seed)
    ctr, rings, vel = [], [], []
    for k in range(M):
        c = np.float32(rng.uniform(0.0, side, 2))
        yaw = rng.uniform(0.0, 2.0 * np.pi)
        ex, ey = extent[0] + 0.3 * k, extent[1] + 0.1 * k
        ctr.append(c.astype(np.float64))
        rings.append(scenarios.place_ring_f32(c, yaw, scenarios.ring_local_offsets(ex, ey)))
        sp = rng.uniform(0.0, 14.0)
        vel.append(_r32([sp * np.cos(yaw), sp * np.sin(yaw)]))
    return ctr, rings, np.array(vel).reshape(M, 2)


class _Crowd:
    """One step's inputs in the fp32 values the device sees, in both forms the step path takes."""

    def __init__(self, n, seed, z_spread, full):
        sc = scenarios.make_scenario(n, seed, n_borders=12 if full else 0, n_static=6 if full else 0, z_spread=z_spread,
                                     border_len=(3.0, 15.0))
        rng = np.random.default_rng(seed + 1)
        self.n, self.sc, self.full = n, sc, full
        self.loc, self.vel, self.wp, self.ts = sc.loc, sc.vel, sc.waypoint, sc.target_speed
        self.radius = _r32(rng.uniform(0.2, 0.45, n)) if full else sc.radius
        self.off = (rng.random(n) < 0.15) if full else np.zeros(n, bool)
        self.side = sc.world_side

    def records(self, extra=5, dtype=PED_STATE_DTYPE):
        rec = np.zeros(self.n + extra, dtype=dtype)
        n = self.n
        rec['loc'][:n], rec['vel'][:n], rec['next_waypoint'][:n] = self.loc, self.vel, self.wp
        rec['radius'][:n], rec['target_speed'][:n] = self.radius, self.ts
        return rec

    def rows(self):
        r = np.full((self.n, 9), np.nan, np.float32)
        r[:, 0:2], r[:, 2:4], r[:, 4:6] = self.loc[:, :2], self.vel[:, :2], self.wp[:, :2]
        r[:, 6], r[:, 7], r[:, 8] = self.ts, self.radius, self.off
        return r

    def zvz(self, planar):
        return None if planar else np.ascontiguousarray(np.stack([self.loc[:, 2], self.vel[:, 2]], axis=1), dtype=np.float32)


def _geom(sc, vehicles):
    ctr, rings, vel = vehicles
    return O.Geometry(sc.borders, sc.border_centers, sc.border_lengths, sc.static_obstacles, list(zip(ctr, rings)),
                      vel if len(ctr) else np.zeros((0, 2)))


def _check(v, loc, vel, wp, ts, radius, off, cfg, geom, blocks, stats, tag):
    """v' of rows ``blocks`` against the C oracle on the same fp32 inputs: the plain 1e-5 bound, the conditioned one with vehicles
    (at most max(2, n / 100) rows leaning on it, as in test_batch_gpu.py).  Records the worst |dv'| / |v'| under ``tag``."""
    prm = O.OracleParams.from_config(cfg)
    vehicles = cfg["forces"].get("dynamic_obstacle_force", False) and len(geom.dynamic_obstacles) > 0
    geo = any(cfg["forces"].get(f, False) for f in ("border_force", "static_obstacle_force", "dynamic_obstacle_force"))
    tie = P.geometry_tie_exposure(O, loc, vel, wp, ts, radius, off, geom, prm) if geo else np.zeros(len(loc))
    needed = 0
    for r in blocks:
        with np.errstate(all="ignore"):
            _, _, v_new, expo, absum = c_oracle.tick(loc, vel, wp, ts, radius, off, geom, prm, DT, rows=r, theta_tol=P.THETA_TOL)
        sl = slice(*r)
        expo = expo + tie[sl]
        if vehicles:
            needed += P.check_velocity_conditioned(v[sl], v_new, expo, absum, DT)
        else:
            P.check_velocity(v[sl], v_new, expo, DT)
        ok = ~np.isnan(v_new).any(axis=1)
        if ok.any():
            rel = np.linalg.norm(v[sl][ok] - v_new[ok], axis=1) / np.maximum(np.linalg.norm(v_new[ok], axis=1), 1e-12)
            k = int(np.argmax(rel))
            stats[tag] = max(stats.get(tag, (0.0,)), (float(rel[k]), len(loc), bool(expo[ok][k] > 0)))     # (worst, at N, exposure row)
    assert needed <= max(2, len(loc) // 100), f"{tag}: {needed} rows needed the conditioned bound"


def _stats_line(title, stats):
    return f"{title}: " + "; ".join(f"{t}: {w:.3g} at N={n}{' (exposure row)' if e else ''}" for t, (w, n, e) in stats.items())


def _blocks(n):
    return ((0, n),) if n <= 4097 else ((0, 128), (n // 2 - 64, n // 2 + 64), (n - 128, n))


def _path(eng, n):
    """What the last step ran: the kernel variant, whether the tile-pair list was on (symmetric path), whether the upload re-packed."""
    v = eng.kernel_variant()
    if "sym" in v:
        items, _ = eng.pair_work()
        n_t = (n + 63) // 64
        v += " list" if items < n_t * (n_t - 1) // 2 + (n_t + 1) // 2 else " grid"
    return v + (" re-packed" if n >= 2048 else " unordered")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _engine(cfg, cw, vehicles):
    eng = SfmEngine(cfg, DT)
    if cw.full:
        eng.set_borders(cw.sc.borders, cw.sc.border_centers, cw.sc.border_lengths)
        eng.set_static_obstacles(cw.sc.static_obstacles)
        eng.set_dynamic_obstacles(list(zip(vehicles[0], vehicles[1])), vehicles[2])
    return eng


# ---- a. oracle parity across the planner's thresholds -------------------------------------------------------------------------------
@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_step_paths_match_the_oracle_at_every_threshold(z_spread):
    planar = z_spread == 0.0
    paths, stats = {}, {}
    for n in SIZES:
        full = n in FULL
        cw = _Crowd(n, 7000 + n, z_spread, full)
        cfg = default_sfm_config(scenarios.ALL_FORCES if full else PED_ONLY)
        cfg["use_ped_radius"] = full
        veh = _vehicles(3, 8000 + n, cw.side) if full else ([], [], np.zeros((0, 2)))
        a, b = _engine(cfg, cw, veh), _engine(cfg, cw, veh)
        try:
            rows, v_pk = cw.rows(), np.full((n, 3), np.nan, np.float32)
            a.step_packed(rows, cw.zvz(planar), v_pk)
            path = _path(a, n)
            rec, v_rc = cw.records(), np.full((n, 3), np.nan, np.float32)
            assert b.step_records(rec, n, cw.off, v_rc) == planar
            assert _path(b, n) == path, (n, path, _path(b, n))
        finally:
            a.close(); b.close()
        assert np.array_equal(_bits(v_pk), _bits(v_rc)), f"N={n}: step_records and step_packed differ"
        assert np.isfinite(v_pk).all(), f"N={n}: v' not fully written"
        if planar:
            assert (v_pk[:, 2] == 0.0).all()
        paths[n] = path
        _check(v_pk, cw.loc, cw.vel, cw.wp, cw.ts, cw.radius, cw.off, cfg, _geom(cw.sc, veh), _blocks(n), stats, path)
    print(f"\nstep paths ({'planar' if planar else '3-D'}): " + "; ".join(f"N={n}: {p}" for n, p in paths.items()))
    print(_stats_line("worst |dv'|/|v'| per path", stats))
    # the planner's choices as observed on the MI355X: the ordered kernel (one launch) below 256 pedestrians, the symmetric pair kernel
    # and its epilogue (two launches) from 256, the spatial re-pack from 2048, the tile-pair list above 4096
    z3 = "false" if planar else "true"
    for n, p in paths.items():
        if n < 256:
            want = f"sfm_tick_kernel<1,{z3},{'true' if n in FULL else 'false'},4> unordered"
        else:
            want = "sfm_pair_sym_kernel+sfm_sym_epilogue_kernel " + ("list" if n > 4096 else "grid") + (" re-packed" if n >= 2048 else " unordered")
        assert p == want, (n, p, want)


# ---- b. one engine, a CARLA-like call sequence ----------------------------------------------------------------------------------------
def test_one_engine_through_a_carla_like_call_sequence():
    """One engine, every call with fresh owning arrays pre-filled with NaN -- N 4200 -> 300 -> 2100 -> 4200 -> 50 -> 0 -> 1 -> 3000,
    planar and 3-D by turns, vehicles 3 -> 0 -> 8 -> 3 with other ring lengths, through set_dynamic_vehicles and set_dynamic_obstacles
    -- then prefixes of one kept buffer (the facade's pattern).  Every array stays alive to the end, so a stale address can only
    produce a wrong answer.  (The first call is the largest crowd, so a stale address also stays inside live memory.)"""
    cfg = default_sfm_config(scenarios.ALL_FORCES)
    cfg["use_ped_radius"] = True
    eng = SfmEngine(cfg, DT)
    keep, stats = [], {}
    big = _Crowd(4200, 123, 0.0, True)
    eng.set_borders(big.sc.borders, big.sc.border_centers, big.sc.border_lengths)
    eng.set_static_obstacles(big.sc.static_obstacles)
    side = big.side
    seq = [  # (N, z_spread, vehicle update)
        (4200, 1.5, ("vehicles", _vehicles(3, 1, side))),
        (300, 0.0, ("vehicles", _vehicles(3, 2, side))),
        (2100, 1.5, None),
        (4200, 0.0, ("obstacles", ([], [], np.zeros((0, 2))))),
        (50, 1.5, ("obstacles", _vehicles(8, 3, side, (3.0, 1.2)))),
        (0, 0.0, None),
        (1, 1.5, ("vehicles", _vehicles(8, 4, side, (3.0, 1.2)))),
        (3000, 0.0, ("vehicles", _vehicles(3, 5, side, (1.5, 0.8)))),
    ]
    veh = ([], [], np.zeros((0, 2)))
    try:
        for k, (n, z_spread, upd) in enumerate(seq):
            if upd is not None:
                veh = upd[1]
                if upd[0] == "vehicles":
                    eng.set_dynamic_vehicles(veh[0], veh[1], veh[2])
                else:
                    eng.set_dynamic_obstacles(list(zip(veh[0], veh[1])) or None, veh[2] if len(veh[0]) else None)
            cw = _Crowd(n, 500 + k, z_spread, True)
            cw.sc.borders, cw.sc.border_centers, cw.sc.border_lengths = big.sc.borders, big.sc.border_centers, big.sc.border_lengths
            cw.sc.static_obstacles = big.sc.static_obstacles
            planar = z_spread == 0.0 or n == 0
            rows, v_pk = cw.rows(), np.full((n, 3), np.nan, np.float32)
            eng.step_packed(rows, cw.zvz(planar), v_pk)
            rec, v_rc = cw.records(), np.full((n, 3), np.nan, np.float32)
            assert eng.step_records(rec, n, cw.off.astype(np.uint8), v_rc) == planar
            keep += [rows, v_pk, rec, v_rc]
            assert np.isfinite(v_pk).all() and np.isfinite(v_rc).all(), f"call {k} (N={n}): v' not fully written"
            assert np.array_equal(_bits(v_pk), _bits(v_rc)), f"call {k} (N={n})"
            if n:
                _check(v_pk, cw.loc, cw.vel, cw.wp, cw.ts, cw.radius, cw.off, cfg, _geom(cw.sc, veh), _blocks(n), stats, f"call {k}")
        # the facade's pattern: prefixes of one kept buffer, a smaller crowd after a larger one
        buf_rows, buf_out = np.full((5000, 9), np.nan, np.float32), np.full((5000, 3), np.nan, np.float32)
        for k, n in enumerate((2500, 700)):
            cw = _Crowd(n, 900 + k, 0.0, True)
            cw.sc.borders, cw.sc.border_centers, cw.sc.border_lengths = big.sc.borders, big.sc.border_centers, big.sc.border_lengths
            cw.sc.static_obstacles = big.sc.static_obstacles
            buf_rows[:n] = cw.rows()
            eng.step_packed(buf_rows[:n], None, buf_out[:n])
            assert np.isfinite(buf_out[:n]).all()
            _check(buf_out[:n], cw.loc, cw.vel, cw.wp, cw.ts, cw.radius, cw.off, cfg, _geom(cw.sc, veh), _blocks(n), stats, f"prefix {k}")
    finally:
        eng.close()
    print("\n" + _stats_line("CARLA-like sequence, worst |dv'|/|v'|", stats))


# ---- c. the facade through the thresholds ----------------------------------------------------------------------------------------------
def _report(vehicles, ids):
    ctr, rings, vel = vehicles
    M = len(ctr)
    return (list(ids[:M]), ctr, [0.0] * M, [v for v in vel], [np.array([2.4, 1.0])] * M, rings)


def test_facade_loop_through_the_thresholds(monkeypatch):
    """Two PedestrianSimulations, one on sfm_step_records and one on sfm_step_packed, driven in lockstep: pedestrians spawned in bulk and
    removed between ticks so that N passes 2048 and 4096, vehicles reported with a changing count (an empty report keeps the last
    vehicles, as in the reference), some pedestrians crossing (border force off).  Every tick: v' by name against the oracle on the
    records the facade held at that tick, and the two simulations bit for bit."""
    pool = scenarios.make_scenario(6000, 4321, n_borders=16, n_static=8, border_len=(3.0, 15.0))
    rng = np.random.default_rng(99)
    radius = _r32(rng.uniform(0.2, 0.45, pool.n))
    cfg = default_sfm_config(scenarios.ALL_FORCES)
    cfg["use_ped_radius"] = True
    info = [[pool.border_centers[k], float(pool.border_lengths[k])] for k in range(len(pool.borders))]
    sims = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SFM_FACADE_RECORDS", flag)
        sims[flag] = PedestrianSimulation(pool.borders, info, pool.static_obstacles, cfg, DT)
        sims[flag].record_states = False
        assert sims[flag]._use_records == (flag == "1")
    prm_geom = dict(borders=pool.borders, centers=pool.border_centers, lengths=pool.border_lengths, static=pool.static_obstacles)
    side = pool.world_side
    plan = [  # (spawn up to, remove every k-th, vehicle report)
        (1500, 0, _vehicles(3, 11, side)),
        (2300, 0, _vehicles(5, 12, side)),
        (2300, 9, None),                                  # 2300 - 256 = 2044: below the re-pack threshold again
        (4300, 0, ([], [], np.zeros((0, 2)))),            # an empty report: the last vehicles stay
        (4300, 31, _vehicles(2, 13, side, (3.0, 1.2))),
        (4700, 0, _vehicles(4, 14, side)),
    ]
    spawned, held, stats = 0, ([], [], np.zeros((0, 2))), {}
    try:
        for t, (upto, every, report) in enumerate(plan):
            for sim in sims.values():
                for i in range(spawned, upto):
                    name = f"p{i}"
                    mm = PedModeManager(name, float(pool.target_speed[i]), PedMode.WALKING_SIDEWALK, 1.5, 1.5)
                    if i % 11 == 0:
                        mm.set_mode(PedMode.CROSSING_ROAD)
                    sim.spawn_pedestrian((name, i, pool.loc[i], pool.vel[i], pool.waypoint[i], mm, float(radius[i]),
                                          float(pool.target_speed[i])))
                if every:
                    for name in list(sim.peds.name()[::every]):
                        sim.peds.remove_pedestrian(name)
                if report is not None:
                    sim.update_dynamic_obstacles(_report(report, list(range(100, 110))))
            spawned = max(spawned, upto)
            if report is not None and len(report[0]):
                held = report
            a, b = sims["1"], sims["0"]
            assert np.array_equal(a.peds.name(), b.peds.name())
            loc, vel, wp = (_r32(a.peds.state[f]) for f in ("loc", "vel", "next_waypoint"))
            names = a.peds.name().copy()
            for sim in sims.values():
                sim.tick(t * DT)
            ts = _r32(a.peds.target_speed())
            off = np.array([m.current_mode in BORDER_FREE_MODES for m in a.peds.mode()])
            rad = _r32(a.peds.radius())
            va, vb = a.get_new_velocities(), b.get_new_velocities()
            assert list(va['id']) == [int(s[1:]) for s in names] and np.array_equal(va['id'], vb['id'])
            assert np.array_equal(va['vel'], vb['vel']), f"tick {t}: records and packed facades differ"
            n = len(names)
            geom = O.Geometry(prm_geom["borders"], prm_geom["centers"], prm_geom["lengths"], prm_geom["static"],
                              list(zip(held[0], held[1])), held[2])
            _check(np.asarray(va['vel']), loc, vel, wp, ts, rad, off, cfg, geom, _blocks(n), stats, f"tick {t} N={n}")
            for sim in sims.values():                      # the CARLA side moves the walkers
                s = sim.peds.state
                s['loc'] = _r32(s['loc'] + DT * s['vel'])
    finally:
        for sim in sims.values():
            sim.close()
    print("\n" + _stats_line("facade loop, worst |dv'|/|v'|", stats))


# ---- d. record layouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_step_records_layouts(z_spread):
    """Records inside a wider structured dtype (stride 132 + 21, every field shifted), a records[::2] view with NaN rows between, and a
    negative-stride view (refused): the first two give step_packed's v' bit for bit."""
    planar = z_spread == 0.0
    n = 300
    cw = _Crowd(n, 77, z_spread, True)
    cfg = default_sfm_config(scenarios.ALL_FORCES)
    cfg["use_ped_radius"] = True
    veh = _vehicles(3, 78, cw.side)
    ref = np.full((n, 3), np.nan, np.float32)
    e = _engine(cfg, cw, veh)
    try:
        e.step_packed(cw.rows(), cw.zvz(planar), ref)
    finally:
        e.close()
    wide = cw.records(dtype=[("pad", "u1", (13,))] + PED_STATE_DTYPE + [("tail", "f8")])
    assert wide.dtype.itemsize == np.dtype(PED_STATE_DTYPE).itemsize + 21
    doubled = np.zeros(2 * n, dtype=PED_STATE_DTYPE)
    for f in ("loc", "vel", "next_waypoint", "radius", "target_speed"):
        doubled[f][1::2] = np.nan
    base = cw.records(extra=0)
    doubled[0::2] = base
    for what, rec in (("wider dtype", wide), ("records[::2]", doubled[::2])):
        e = _engine(cfg, cw, veh)
        try:
            v = np.full((n, 3), np.nan, np.float32)
            assert e.step_records(rec, n, cw.off, v) == planar
            assert np.array_equal(_bits(v), _bits(ref)), what
        finally:
            e.close()
    e = _engine(cfg, cw, veh)
    try:
        with pytest.raises(SfmLibraryError):
            e.step_records(base[::-1], n, cw.off, np.zeros((n, 3), np.float32))
    finally:
        e.close()


def test_step_records_nan_z_takes_the_3d_path():
    """planar_tolerance = 0.05 on nearly flat ground with one NaN z: the NumPy rule of the packed facade path says 3-D (max |z - median|
    is NaN), so sfm_step_records must too, with step_packed's 3-D v' bit for bit, NaN rows included."""
    n = 200
    cw = _Crowd(n, 31, 0.0, False)
    rng = np.random.default_rng(32)
    cw.loc[:, 2] = _r32(0.2 + rng.uniform(-0.004, 0.004, n))
    cw.vel[:, 2] = _r32(rng.uniform(-1e-3, 1e-3, n))
    cw.loc[17, 2] = np.nan
    cfg = default_sfm_config(PED_ONLY)
    a, b = SfmEngine(cfg, DT), SfmEngine(cfg, DT)
    try:
        v_rc, v_pk = np.full((n, 3), 7.0, np.float32), np.full((n, 3), 7.0, np.float32)
        assert a.step_records(cw.records(), n, None, v_rc, planar_tolerance=0.05) is False
        b.step_packed(cw.rows(), cw.zvz(False), v_pk)
    finally:
        a.close(); b.close()
    assert (v_pk != 7.0).all()                                  # (NaN != 7: every row written)
    assert np.array_equal(_bits(v_rc), _bits(v_pk))


# ---- e. dynamic_obstacles() after a change of M ---------------------------------------------------------------------------------------
def _assert_rings(got, ctr, rings):
    assert len(got) == len(rings)
    for (c_g, r_g), c, r in zip(got, ctr, rings):
        assert np.array_equal(c_g, _r32(np.asarray(c)[:2])) and np.array_equal(r_g, _r32(r))


def test_dynamic_obstacles_after_fewer_vehicles():
    eng = SfmEngine(default_sfm_config(scenarios.ALL_FORCES), DT)
    try:
        eng.set_dynamic_boxes([np.array([3.0 * k, 1.0]) for k in range(10)], np.zeros(10), np.full((10, 2), [2.4, 1.0]), np.zeros((10, 2)))
        assert len(eng.dynamic_obstacles()) == 10
        c, r, v = _vehicles(3, 40, 50.0)
        eng.set_dynamic_obstacles(list(zip(c, r)), v)
        _assert_rings(eng.dynamic_obstacles(), c, r)
    finally:
        eng.close()


def test_dynamic_obstacles_after_more_vehicles():
    eng = SfmEngine(default_sfm_config(scenarios.ALL_FORCES), DT)
    try:
        c, r, v = _vehicles(3, 41, 50.0)
        eng.set_dynamic_vehicles(c, r, v)
        _assert_rings(eng.dynamic_obstacles(), c, r)
        c10, r10, v10 = _vehicles(10, 42, 50.0, (3.5, 1.5))
        eng.set_dynamic_obstacles(list(zip(c10, r10)), v10)
        _assert_rings(eng.dynamic_obstacles(), c10, r10)
        c3, r3, v3 = _vehicles(3, 43, 50.0)                      # the packed report again, with the ring sizes it kept
        eng.set_dynamic_vehicles(c3, r3, v3)
        _assert_rings(eng.dynamic_obstacles(), c3, r3)
        eng.set_dynamic_vehicles([], [], None)
        assert eng.dynamic_obstacles() == []
    finally:
        eng.close()
