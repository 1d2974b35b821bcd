"""The per-force 1e-5 parity (``P.check_force``'s bound) for the two kernels that cannot record their forces: sfm_fused_tick_kernel
(every device-resident run; the kernel bench.py times) and sfm_batch_tick_kernel.

A tick at dt = 1 with max_speed_factor = 1e4 (the cap cannot act) gives v' = v + F up to one fp32 rounding, so
``P.check_force_from_velocity`` reads F back as (v' - v) / dt and holds it to |dF_i| <= 1e-5 max(|F_i|, A_i) + exposure_i plus a
floor of 2^-23 |v'| / dt for that rounding -- one force family at a time (waypoint redraws off), and all five on the total.

Fused tick, both roles of its pair work:  mode 0 -- run(1) from a fresh upload, pairs of the launch in front;  mode 1 -- the second
tick of run(2), pairs computed inside the integrating launch, compared with the oracle stepping from S1 (a twin handle's run(1):
a run does not depend on how the caller cuts it into calls).  Run with  python -m pytest tests/test_force_readback_gpu.py -m gpu -s."""
import copy

import numpy as np
import pytest

import _parity as P
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd.batch import SfmBatch
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.engine import SfmEngine
from oracle import c_oracle
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

DT = 1.0
MSF = 1e4
PED = ("pedestrian_force",)
FAMILIES = {"pedestrian": PED, "border": ("border_force",), "static": ("static_obstacle_force",),
            "dynamic": ("dynamic_obstacle_force",), "all5": scenarios.ALL_FORCES}


def _cfg(forces, use_radius=False, ped_A=None):
    cfg = default_sfm_config(forces)
    cfg["max_speed_factor"] = MSF
    cfg["use_ped_radius"] = bool(use_radius)
    if ped_A is not None:
        cfg["pedestrian_force"]["A"] = ped_A
    return cfg


def _fused_geometry_cfg(family, use_radius=False):
    """A geometry family alone through the fused tick.  Without the pedestrian force a run takes the ordered kernel (which records
    its forces and is held to check_force elsewhere); with it on at A = 0 the run takes sfm_fused_tick_kernel and the geometry
    family is the only force left."""
    if family == "all5":
        return _cfg(scenarios.ALL_FORCES, use_radius)
    return _cfg(PED + FAMILIES[family], use_radius, ped_A=0.0)


def _geometry(sc):
    return O.Geometry(sc.borders, sc.border_centers, sc.border_lengths, sc.static_obstacles, sc.dynamic_obstacles, sc.dynamic_vel)


def _readback(name, v_dev, loc, vel, sc, crossing, geom, prm, geo):
    """Oracle forces on the fp32 state (loc, vel) -> check_force_from_velocity of the device's v'."""
    with np.errstate(all="ignore"):
        _, total, _, expo, absum = c_oracle.tick(loc, vel, sc.waypoint, sc.target_speed, sc.radius, crossing, geom, prm, DT,
                                                 theta_tol=P.THETA_TOL)
    if geo:
        expo = expo + P.geometry_tie_exposure(O, loc, vel, sc.waypoint, sc.target_speed, sc.radius, crossing, geom, prm)
    return P.check_force_from_velocity(name, v_dev, vel, DT, total, absum, expo, sc.target_speed * MSF)


def _engine(sc, cfg, crossing, geo):
    eng = SfmEngine(cfg, DT)
    if geo:
        eng.set_borders(sc.borders, sc.border_centers, sc.border_lengths)
        eng.set_static_obstacles(sc.static_obstacles)
        if len(sc.dynamic_obstacles):
            eng.set_dynamic_boxes([c for c, _ in sc.dynamic_obstacles], sc.dynamic_yaw, sc.dynamic_extent, sc.dynamic_vel)
    eng.upload_state(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, crossing)
    return eng


def _both_roles(sc, cfg, label, monkeypatch, crossing=None, geo=False):
    """Mode 0 and mode 1 of sfm_fused_tick_kernel against the oracle, force by force.  Returns the printed summary line."""
    n = sc.n
    monkeypatch.setenv("SFM_FUSED", "1")
    if n > 4096:
        monkeypatch.setenv("SFM_CUTOFF", "0")                 # (above 4096 the list cutoff, and with it the two-launch tick, is the default)
    crossing = np.zeros(n, bool) if crossing is None else crossing
    prm = O.OracleParams.from_config(cfg)
    twin = _engine(sc, cfg, crossing, geo)
    try:
        twin.run(1)
        assert "fused" in twin.kernel_variant(), twin.kernel_variant()
        loc1, vel1, _ = twin.state()
        veh1 = twin.dynamic_obstacles() if geo and len(sc.dynamic_obstacles) else []
        planar = twin.planar
    finally:
        twin.close()
    eng = _engine(sc, cfg, crossing, geo)
    try:
        eng.run(2)
        assert "fused" in eng.kernel_variant(), eng.kernel_variant()
        v2 = eng.velocities()
    finally:
        eng.close()
    if planar:                                                # S1 inside a run of two ticks is the twin's S1, bit for bit
        rec = _engine(sc, cfg, crossing, geo)
        try:
            frames, _ = rec.run_recorded(2)
        finally:
            rec.close()
        want = np.float32(np.stack([loc1[:, 0], loc1[:, 1], vel1[:, 0], vel1[:, 1]], axis=1))
        assert np.array_equal(frames[1], want, equal_nan=True), "frame 1 of run_recorded(2) is not the twin's S1"
    w0, f0 = _readback(f"{label} mode 0", vel1, sc.loc, sc.vel, sc, crossing, _geometry(sc), prm, geo)
    sc1 = copy.deepcopy(sc)
    if len(sc.dynamic_obstacles) and cfg["forces"]["dynamic_obstacle_force"]:
        scenarios.advance_dynamic(sc1, DT)                    # the integrating launch moved the vehicles on by dt = 1
        for (c_d, r_d), (c_h, r_h) in zip(veh1, sc1.dynamic_obstacles):
            assert np.array_equal(c_d, c_h) and np.array_equal(r_d, r_h), "vehicles after tick 1"
    w1, f1 = _readback(f"{label} mode 1", v2, loc1, vel1, sc1, crossing, _geometry(sc1), prm, geo)
    line = (f"fused readback {label}: worst |dF|/max(|F|,A) mode 0 {w0:.2e} mode 1 {w1:.2e}; rows on the fp32 floor {f0} + {f1} "
            f"of {2 * n}")
    print("\n" + line)
    return line


# ---- pedestrian force alone ------------------------------------------------------------------------------------------------------
PLANAR_SIZES = [2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2047, 2048, 2049, 4095, 4096, 4160]


@pytest.mark.parametrize("density", [0.25, 1.0])
@pytest.mark.parametrize("n", PLANAR_SIZES)
def test_fused_pedestrian_force_planar(n, density, monkeypatch):
    """Whole and ragged tiles, odd pair counts (two pairs per lane), the 16-wave and the 8-wave form of the launch."""
    sc = scenarios.make_scenario(n, 9100 + n, density=density)
    _both_roles(sc, _cfg(PED), f"pedestrian planar N={n} density {density}", monkeypatch)


@pytest.mark.parametrize("n", [300, 2048, 4096])
def test_fused_pedestrian_force_planar_with_radius(n, monkeypatch):
    sc = scenarios.make_scenario(n, 9200 + n, density=0.25)
    _both_roles(sc, _cfg(PED, use_radius=True), f"pedestrian planar N={n} use_ped_radius", monkeypatch)


@pytest.mark.parametrize("use_radius", [False, True], ids=["plain", "radius"])
@pytest.mark.parametrize("n", [64, 130, 300, 1000, 4096])
def test_fused_pedestrian_force_3d(n, use_radius, monkeypatch):
    sc = scenarios.make_scenario(n, 9300 + n, density=0.25 if use_radius else 1.0, z_spread=1.5)
    _both_roles(sc, _cfg(PED, use_radius), f"pedestrian 3-D N={n}{' use_ped_radius' if use_radius else ''}", monkeypatch)


# ---- constructed edge rows -------------------------------------------------------------------------------------------------------
def _edge_scene(z_spread, shift, density=1.0):
    """A random crowd of 256 with pairs built to sit on the decisions of the Moussaid term: theta (= angle(e) - angle(t) - eps B,
    t the direction of D = lambda dv + e) near 0, +-pi/2, +-pi and the raw angle at the +-pi wrap; a coincident pair (different
    velocities: finite in the reference, NaN in the fast body); a pair 1e-3 m apart; in 3-D a pair above one another; rows at rest and
    rows with equal velocities; optionally the whole scene moved to (+350, -280) m."""
    n = 256
    sc = scenarios.make_scenario(n, 9400 + int(z_spread * 10) + int(shift), density=density, z_spread=z_spread)
    loc, vel = sc.loc.copy(), sc.vel.copy()
    ip = O.Interaction.from_table(default_sfm_config(PED)["pedestrian_force"])
    Dn = 1.4
    eB = ip.epsilon * ip.gamma * Dn
    angles = [eB, eB + 3e-6, eB - 3e-6, np.pi / 2, -np.pi / 2, np.pi / 2 + eB, -np.pi / 2 + eB, np.pi - 1e-6, -np.pi + 1e-6,
              -np.pi + eB, np.pi]
    rng = np.random.default_rng(17)
    for k, ang in enumerate(angles):
        i, j = 2 * k, 2 * k + 1
        phi = rng.uniform(0.0, 2.0 * np.pi)
        e = np.array([np.cos(phi), np.sin(phi)])
        loc[j, :2] = loc[i, :2] + 0.6 * e
        loc[j, 2] = loc[i, 2]
        D = Dn * np.array([np.cos(phi - ang), np.sin(phi - ang)])      # angle(e) - angle(D) = ang
        vel[i, :2] = vel[j, :2] + (D - e) / ip.lam
        vel[i, 2] = vel[j, 2]
    loc[41] = loc[40]                                          # coincident, different velocities
    loc[43] = loc[42] + np.array([1e-3, 0.0, 0.0])             # 1e-3 m apart
    if z_spread:
        loc[45] = loc[44] + np.array([0.0, 0.0, 0.5])          # above one another
    vel[50:54] = 0.0                                           # at rest
    loc[56] = loc[55] + np.array([0.5, 0.3, 0.0])
    vel[56] = vel[55]                                          # equal velocities: D = e
    if shift:
        loc[:, :2] += np.array([350.0, -280.0])
        sc.waypoint[:, :2] += np.array([350.0, -280.0])
    sc.loc, sc.vel = np.float32(loc).astype(np.float64), np.float32(vel).astype(np.float64)
    sc.waypoint = np.float32(sc.waypoint).astype(np.float64)
    return sc


@pytest.mark.parametrize("shift", [False, True], ids=["origin", "carla_town"])
@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
@pytest.mark.parametrize("use_radius", [False, True], ids=["plain", "radius"])
def test_fused_constructed_edge_rows(z_spread, shift, use_radius, monkeypatch):
    sc = _edge_scene(z_spread, shift, 0.25 if use_radius else 1.0)     # (overlapping radii at 1 ped/m2: forces near the cap)
    _both_roles(sc, _cfg(PED, use_radius), f"edge rows {'3-D' if z_spread else 'planar'}{' shifted' if shift else ''}"
                f"{' use_ped_radius' if use_radius else ''}", monkeypatch)


# ---- geometry role ---------------------------------------------------------------------------------------------------------------
def _geo_scenario(n, seed, z_spread=0.0):
    return scenarios.make_scenario(n, seed, n_borders=max(24, n // 16), n_static=max(12, n // 128), n_dynamic=6, border_len=(5.0, 25.0),
                                   z_spread=z_spread)


@pytest.mark.parametrize("family", ["border", "static", "dynamic", "all5"])
@pytest.mark.parametrize("n,z_spread", [(64, 0.0), (512, 0.0), (2048, 0.0), (4096, 0.0), (200, 1.5), (1000, 1.5)])
def test_fused_geometry_forces(n, z_spread, family, monkeypatch):
    """Border / static obstacle / device-side vehicle forces each alone (the geometry workgroups of the fused tick; pedestrian force
    at A = 0, see _fused_geometry_cfg), and all five forces compared on the total; a crossing mask switches the border force off for
    every ninth pedestrian."""
    sc = _geo_scenario(n, 9500 + n, z_spread)
    crossing = np.zeros(n, bool)
    crossing[::9] = True
    _both_roles(sc, _fused_geometry_cfg(family), f"{family} N={n}{' 3-D' if z_spread else ''}", monkeypatch, crossing, geo=True)


def test_fused_geometry_at_baseline_c1(monkeypatch):
    sc, forces = scenarios.baseline_scenario("c1")
    assert tuple(forces) == tuple(scenarios.ALL_FORCES)
    _both_roles(sc, _cfg(forces), "BASELINE c1", monkeypatch, geo=True)


@pytest.mark.parametrize("n,n_borders,n_static,use_radius", [(64, 400, 100, False), (200, 1500, 200, True), (64, 4300, 100, False),
                                                             (700, 40, 3000, False)])
def test_fused_geometry_scan_forms(n, n_borders, n_static, use_radius, monkeypatch):
    """The scan forms of test_fused_tick_geometry_scan_forms_pinned_to_the_oracle (on-the-spot scan up to 64 polylines per wave,
    find -> per-wave list -> dealt scan beyond), all five forces."""
    sc = scenarios.make_scenario(n, 6600 + n + n_borders, n_borders=n_borders, n_static=n_static, n_dynamic=6, border_len=(5.0, 25.0),
                                 density=0.25 if use_radius else 1.0)
    _both_roles(sc, _cfg(scenarios.ALL_FORCES, use_radius), f"scan form N={n} {n_borders} borders {n_static} static", monkeypatch,
                geo=True)


# ---- batch kernel ----------------------------------------------------------------------------------------------------------------
BATCH_SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 1023, 1024]
POLY_POINTS = [1, 63, 64, 65, 129]


def _line(start, heading, points, spacing=0.1):
    d = np.array([np.cos(heading), np.sin(heading)])
    return np.float32(start + spacing * np.arange(points)[:, None] * d).astype(np.float64)


def _ring(center, radius, points):
    th = 2.0 * np.pi * np.arange(points) / points
    return np.float32(center + radius * np.column_stack((np.cos(th), np.sin(th)))).astype(np.float64)


def _batch_scene(family, n, k, z_spread):
    sc = vars(scenarios.make_scenario(n, 9700 + 37 * k + n, z_spread=z_spread))
    rng = np.random.default_rng(9800 + k)
    side = max(sc["world_side"], 4.0)
    sc["radius"] = np.float32(rng.uniform(0.2, 0.45, n)).astype(np.float64)
    if n >= 3:
        sc["loc"][1] = sc["loc"][2]                            # a coincident pair (different velocities)
    if z_spread and n >= 5:
        sc["loc"][4, :2] = sc["loc"][3, :2]                    # ... and a pair above one another
        sc["loc"][4, 2] = np.float32(sc["loc"][3, 2] + 0.5)
    if family == "border":
        borders = [_line(rng.uniform(0.0, side, 2), rng.uniform(0.0, 2.0 * np.pi), p) for p in POLY_POINTS]
        borders.append(_line(np.zeros(2), 0.25 * np.pi, 9))   # short, in a corner: only some lanes of a wave keep it
        sc["borders"] = borders
        sc["border_centers"] = np.array([b[len(b) // 2] for b in borders])
        sc["border_lengths"] = np.array([max(len(b), 3) * 0.1 for b in borders])
        sc["crossing"] = rng.random(n) < 0.2
    elif family in ("static", "dynamic"):
        obs = []
        for p in POLY_POINTS:
            c = np.float32(rng.uniform(0.0, side, 2)).astype(np.float64)
            obs.append((c, _ring(c, rng.uniform(0.3, 1.5), p)))
        if family == "static":
            sc["static_obstacles"] = obs
        else:
            sc["dynamic_obstacles"] = obs
            h = rng.uniform(0.0, 2.0 * np.pi, len(obs))
            sc["dynamic_vel"] = np.float32(14.0 * np.column_stack((np.cos(h), np.sin(h)))).astype(np.float64)
    return sc


def _batch_oracle(sc, cfg):
    n = len(sc["loc"])
    prm = O.OracleParams.from_config(cfg)
    geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"], sc["dynamic_obstacles"],
                      sc["dynamic_vel"])
    crossing = sc.get("crossing")
    crossing = np.zeros(n, bool) if crossing is None else crossing
    with np.errstate(all="ignore"):
        _, total, _, expo, absum = c_oracle.tick(sc["loc"], sc["vel"], sc["waypoint"], sc["target_speed"], sc["radius"], crossing, geom,
                                                 prm, DT, theta_tol=P.THETA_TOL)
    expo = expo + P.geometry_tie_exposure(O, sc["loc"], sc["vel"], sc["waypoint"], sc["target_speed"], sc["radius"], crossing, geom, prm)
    return total, expo, absum


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_batch_kernel_force_by_force(z_spread):
    """One batch: every size of BATCH_SIZES (S = 4 / 2 / 1 j-slices, one pass and several) with each force family alone -- the
    pedestrian force, borders (1 .. 129 points and a polyline only some lanes keep, crossing masks), static obstacles, vehicles at
    14 m/s -- radius on in alternate scenes, a coincident pair and in 3-D a pair above one another."""
    scenes, cfgs, tags = [], [], []
    for family in ("pedestrian", "border", "static", "dynamic"):
        for n in BATCH_SIZES:
            k = len(scenes)
            scenes.append(_batch_scene(family, n, k, z_spread))
            cfgs.append(_cfg(FAMILIES[family], use_radius=k % 2))
            tags.append(f"{family} N={n}")
    b = SfmBatch(cfgs, [DT] * len(scenes))
    try:
        b.upload(scenes)
        assert b.planar == (z_spread == 0.0)
        b.tick(integrate=False)
        states = b.state()
    finally:
        b.close()
    worst, floor, rows = {}, {}, {}
    for sc, cfg, tag, (loc, vel) in zip(scenes, cfgs, tags, states):
        np.testing.assert_array_equal(loc, np.float32(sc["loc"]))
        total, expo, absum = _batch_oracle(sc, cfg)
        w, f = P.check_force_from_velocity(f"batch {tag}", vel, sc["vel"], DT, total, absum, expo, sc["target_speed"] * MSF)
        fam = tag.split()[0]
        worst[fam] = max(worst.get(fam, 0.0), w)
        floor[fam] = floor.get(fam, 0) + f
        rows[fam] = rows.get(fam, 0) + len(sc["loc"])
    for fam in worst:
        print(f"\nbatch readback {'3-D' if z_spread else 'planar'} {fam}: worst |dF|/max(|F|,A) {worst[fam]:.2e}; rows on the fp32 "
              f"floor {floor[fam]} of {rows[fam]}")


def test_batch_3d_integrating_run():
    """test_multi_tick_runs in 3-D: 20 integrating ticks at dt = 0.05 with the cap on, re-synchronised every tick against
    O.free_step(round_f32=True): v' through check_velocity, x' (z included) to 1e-6."""
    geo = ("acceleration_force", "pedestrian_force", "border_force", "static_obstacle_force")
    scenes = []
    for k, n in enumerate((50, 200, 7)):
        sc = vars(scenarios.make_scenario(n, 9900 + k, n_borders=6 if k < 2 else 0, n_static=3 if k < 2 else 0, z_spread=1.5,
                                          border_len=(3.0, 15.0)))
        sc["radius"] = np.float32(np.random.default_rng(k).uniform(0.2, 0.45, n)).astype(np.float64)
        if k == 1:
            sc["crossing"] = np.random.default_rng(5).random(n) < 0.2
        scenes.append(sc)
    cfgs = [default_sfm_config(geo if k < 2 else ("acceleration_force", "pedestrian_force")) for k in range(3)]
    cfgs[1]["use_ped_radius"] = True
    dt = 0.05
    b = SfmBatch(cfgs, dt)
    try:
        b.upload(scenes)
        assert not b.planar
        cur = [(np.float32(sc["loc"]).astype(np.float64), np.float32(sc["vel"]).astype(np.float64)) for sc in scenes]
        for t in range(20):
            b.tick(integrate=True)
            got = b.state()
            for k, (sc, cfg) in enumerate(zip(scenes, cfgs)):
                n = len(sc["loc"])
                loc, vel = cur[k]
                prm = O.OracleParams.from_config(cfg)
                geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"], [], None)
                crossing = sc.get("crossing")
                crossing = np.zeros(n, bool) if crossing is None else crossing
                diag = {}
                with np.errstate(all="ignore"):
                    oloc, ovel, _, _ = O.free_step(loc, vel, sc["waypoint"], sc["target_speed"], sc["radius"], crossing,
                                                   np.zeros(n, np.int64), geom, prm, dt, redraw=False, round_f32=True)
                    O.tick_forces(loc, vel, sc["waypoint"], sc["target_speed"], sc["radius"], crossing, geom, prm,
                                  theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
                dloc, dvel = got[k]
                P.check_velocity(dvel, ovel, diag["total"][0], dt)
                assert np.max(np.abs(dloc - oloc)) <= 1e-6 * max(1.0, np.max(np.abs(oloc))) + 1e-6, f"scene {k} tick {t}"
                assert np.ptp(dloc[:, 2]) > 0.0                # the z spread is kept
                cur[k] = (dloc, dvel)
    finally:
        b.close()


def test_lifted_planar_batch_keeps_its_z():
    """A planar batch whose common z is 1.5 keeps z = 1.5 through run(5), and steps x, y, v exactly as at z = 0."""
    scenes = [vars(scenarios.make_scenario(n, 9950 + n, n_borders=4, n_static=2, border_len=(3.0, 15.0))) for n in (1, 40, 300)]
    lifted = copy.deepcopy(scenes)
    for sc in lifted:
        sc["loc"][:, 2] = 1.5
    cfg = default_sfm_config(("acceleration_force", "pedestrian_force", "border_force", "static_obstacle_force"))
    out = []
    for group in (scenes, lifted):
        b = SfmBatch(cfg, 0.05, B=len(group))
        try:
            b.upload(group)
            assert b.planar
            b.run(5)
            out.append(b.state())
        finally:
            b.close()
    for (loc0, vel0), (loc1, vel1) in zip(*out):
        assert (loc1[:, 2] == 1.5).all()
        assert np.array_equal(loc0[:, :2], loc1[:, :2]) and np.array_equal(vel0, vel1)
