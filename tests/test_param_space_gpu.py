"""Every kernel path against the oracle AWAY from the stock parameters (tests/_param_sets.py).

The host folds the parameters into derived constants and into reach bounds that decide which work is skipped; at the stock values
the skipped terms are exactly negligible, so a reach or a constant derived from the wrong value passes every stock test.  One
matrix, parameter set x path.  Each cell: the path is reached through the documented environment knobs and
ASSERTED (kernel_variant / launch count / pair work); the oracle alone must meet the two conditions of tests/_param_cells.py
(exposed rows <= 10 %, max_amp <= 1); then ``_parity.check_force`` force by force where the path records forces,
``check_force_from_velocity`` where it cannot (the fused tick), and ``check_velocity``.  Tolerances are _parity's, unchanged.
Run with  python -m pytest tests/test_param_space_gpu.py -m gpu -s."""
import ctypes as C

import numpy as np
import pytest

import _param_cells as pc
import _param_sets as psets
import _parity as P
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import SfmBatch, batch_params
from carla_social_force_model_amd.engine import SfmEngine, params_from_config
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

ALL_SETS = psets.NAMES
CORE = ("longrange", "shortrange", "epsneg")          # what every path gets at the least
KNOBS = ("SFM_SYM", "SFM_IPW", "SFM_TEAM", "SFM_CUTOFF", "SFM_REORDER", "SFM_FUSED", "SFM_PAIR_GEO", "SFM_GEO_SLICES",
         "SFM_NO_STRAIGHT", "SFM_POOL", "SFM_STRIPS")


def _env(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _engine(sc, cfg, dt, geo=True, crossing=None, boxes=False):
    eng = SfmEngine(cfg, dt)
    if geo:
        if len(sc.borders):
            eng.set_borders(sc.borders, sc.border_centers, sc.border_lengths)
        eng.set_static_obstacles(sc.static_obstacles)
        if boxes and len(sc.dynamic_obstacles):
            eng.set_dynamic_boxes([c for c, _ in sc.dynamic_obstacles], sc.dynamic_yaw, sc.dynamic_extent, sc.dynamic_vel)
        else:
            eng.set_dynamic_obstacles(sc.dynamic_obstacles, sc.dynamic_vel)
    eng.upload_state(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, crossing)
    return eng


def _recorded_tick_cell(label, sc, cfg, dt, expect, literal=True, geo=True, launches=None):
    """One recorded tick: conditions on the oracle, path assertion, every force, the total and v'."""
    ref = pc.Ref(sc.loc, sc.vel, sc, cfg, dt)
    share, amp = ref.conditions(label, literal)
    eng = _engine(sc, cfg, dt, geo)
    try:
        eng.tick(record=True)
        variant = eng.kernel_variant()
        assert expect(variant), (label, variant)
        if launches is not None:
            assert eng.timing()[2] == launches, (label, eng.timing())
        worst = ref.check_forces(label, eng.forces)
        vw = ref.check_velocity(eng.velocities())
        work = eng.pair_work() if "sym" in variant else None
    finally:
        eng.close()
    print(f"\n{label}: {variant}  exposed {share:.1%}  max_amp {amp:.3g}  worst err/scale {worst:.2e}  v' rel {vw:.2e}")
    return work


# ---- ordered sfm_tick_kernel ------------------------------------------------------------------------------------------------------
ORDERED = [(name, 0.0) for name in ALL_SETS] + [(name, 1.5) for name in CORE]


@pytest.mark.parametrize("name,z_spread", ORDERED, ids=[f"{a}-{'3d' if b else 'planar'}" for a, b in ORDERED])
def test_ordered_tick_kernel(name, z_spread, monkeypatch):
    """SFM_SYM=0 at 2 rows per wave, teams of 4 (the default is picked by size), all five forces, use_ped_radius on."""
    _env(monkeypatch, SFM_SYM=0, SFM_IPW=2, SFM_TEAM=4)
    sc = pc.scene(700, 5700, z_spread)
    _recorded_tick_cell(f"ordered {name} z={z_spread}", sc, pc.set_config(name, pc.ALL5, rad=True), psets.step_of(name),
                        lambda v: v.startswith("sfm_tick_kernel<2,") and v.endswith(",4>"))


# ---- symmetric pair kernel + epilogue, dense slab -----------------------------------------------------------------------------------
@pytest.mark.parametrize("z_spread,rad", [(0.0, False), (1.5, True)], ids=["planar", "3d-radius"])
@pytest.mark.parametrize("name", ALL_SETS)
def test_symmetric_dense_slab(name, z_spread, rad, monkeypatch):
    _env(monkeypatch, SFM_SYM=1, SFM_CUTOFF=0)
    sc = pc.scene(1000, 6000, z_spread)
    if name == "shortrange":                           # one coincident pair (equal velocities: NaN rows on both sides) and one with
        sc.loc[70] = sc.loc[3]; sc.vel[70] = sc.vel[3]  # different velocities (finite), in different tiles
        sc.loc[200] = sc.loc[900]
    work = _recorded_tick_cell(f"sym dense {name} z={z_spread}", sc, pc.set_config(name, pc.ALL5, rad=rad), psets.step_of(name),
                               lambda v: "sym" in v)
    n_t = (sc.n + 63) // 64
    assert work[0] == n_t * (n_t - 1) // 2 + (n_t + 1) // 2          # the 2-D grid: no list, nothing dropped


# ---- geometry: stand-alone sfm_geometry_kernel and the geometry workgroups of sfm_pair_geo_kernel -----------------------------------
GEO_FORMS = [("pairgeo", None, False), ("pairgeo", None, True), ("alone", 1, False), ("alone", 1, True), ("alone", 8, False),
             ("alone", 8, True)]
# every form at longrange and shortrange; one pair-launch form and two stand-alone forms at eps0 and lam0
GEO_CELLS = [(name,) + f for name in ("longrange", "shortrange") for f in GEO_FORMS]
GEO_CELLS += [(name,) + f for name in ("eps0", "lam0") for f in (GEO_FORMS[0], GEO_FORMS[2], GEO_FORMS[3])]


@pytest.mark.parametrize("name,form,slices,no_straight", GEO_CELLS,
                         ids=[f"{a}-{f}-s{s}-{'scan' if n else 'shortcut'}" for a, f, s, n in GEO_CELLS])
def test_geometry_kernels(name, form, slices, no_straight, monkeypatch):
    """Border / obstacle forces with use_ped_radius on: border_skip and border_nlb from b, the obstacle sets' own folded constants
    and thresholds.  SFM_PAIR_GEO=0: sfm_geometry_kernel in a launch of its own (3 launches per tick), SFM_GEO_SLICES workgroups
    per tile; default: its workgroups inside the pair launch (2 launches).  SFM_NO_STRAIGHT: the straight-border shortcut off."""
    env = {"SFM_SYM": 1, "SFM_CUTOFF": 0}
    if form == "alone":
        env.update(SFM_PAIR_GEO=0, SFM_GEO_SLICES=slices)
    if no_straight:
        env["SFM_NO_STRAIGHT"] = 1
    _env(monkeypatch, **env)
    sc = pc.scene(640, 6400)
    _recorded_tick_cell(f"geometry {form} slices {slices} no_straight {no_straight} {name}", sc,
                        pc.set_config(name, pc.ALL5, rad=True), 0.05, lambda v: "sym" in v, launches=3 if form == "alone" else 2)


# ---- tile-pair list cutoff --------------------------------------------------------------------------------------------------------
def _list_scene(kind):
    if kind == "planar":
        return scenarios.baseline_scenario("c2")[0]              # N = 4096 in grid order: compact tiles, 128 m across
    if kind == "3d":
        return scenarios.make_scenario(4096, 1002, z_spread=1.5)
    return scenarios.make_scenario(98304, 777)                    # dense slab 1.2 GiB > 1 GiB: the row pool takes over


@pytest.mark.parametrize("kind", ["planar", "3d", "pool"])
@pytest.mark.parametrize("name", CORE)
def test_list_cutoff(name, kind, monkeypatch):
    """SFM_CUTOFF=1, rows in the caller's (grid) order.  The list must have something to lose (tests/test_param_space_host.py shows
    on the CPU that a stock reach would drop terms above the tolerance at longrange) and must differ from the stock list:
    strictly fewer pair terms at shortrange, strictly more at longrange, all below N (N - 1) / 2 + N."""
    _env(monkeypatch, SFM_SYM=1, SFM_CUTOFF=1, SFM_REORDER=0)
    sc = _list_scene(kind)
    n = sc.n
    cfg = pc.set_config(name, pc.PED_ACC)
    blocks = [None] if n <= 4096 else [(0, 128), (n // 2 - 64, n // 2 + 64), (n - 128, n)]
    work = {}
    for tag, c in ((name, cfg), ("stock", pc.set_config("stock", pc.PED_ACC))):
        eng = _engine(sc, c, 0.05, geo=False)
        try:
            eng.tick(record=True)
            assert "sym" in eng.kernel_variant(), eng.kernel_variant()
            work[tag] = eng.pair_work()
            if tag == "stock":
                continue
            F = {k: eng.forces(k) for k in ("acceleration_force", "pedestrian_force", "total")}
            v = eng.velocities()
        finally:
            eng.close()
    exposed = sampled = 0
    for rows in blocks:
        ref = pc.Ref(sc.loc, sc.vel, sc, cfg, 0.05, geom=O.Geometry(), rows=rows)
        share, amp = pc.material_share(ref), ref.max_amp
        assert amp <= pc.MAX_AMP, (name, kind, rows, amp)
        exposed, sampled = exposed + share * (ref.rows[1] - ref.rows[0]), sampled + ref.rows[1] - ref.rows[0]
        worst = ref.check_forces(f"list {name} {kind} rows {rows}", lambda k: F[k])
        vw = ref.check_velocity(v)
        print(f"\nlist {name} {kind} rows {rows}: exposed (> ATOL) {share:.1%} (non-zero {ref.share:.1%})  max_amp {amp:.3g}  "
              f"worst {worst:.2e}  v' rel {vw:.2e}  pair work {work[name]} (stock {work['stock']})")
    # the cell's rows are all the sampled rows: those exposed above ATOL <= 10 % of them (_param_cells.Ref.conditions, literal=False)
    assert exposed <= pc.MAX_EXPOSED_SHARE * sampled, (name, kind, exposed, sampled)
    n_t = (n + 63) // 64
    every_item = n_t * (n_t - 1) // 2 + (n_t + 1) // 2
    assert work[name][1] < n * (n - 1) // 2 + n and work["stock"][1] < n * (n - 1) // 2 + n
    assert work["stock"][0] < every_item, "the stock list drops nothing on this crowd: the comparison would be vacuous"
    if name == "shortrange":
        assert work[name][1] < work["stock"][1], work
    if name == "longrange":
        assert work[name][1] > work["stock"][1], work


@pytest.mark.parametrize("name", CORE)
def test_ordered_kernel_with_tile_boxes(name, monkeypatch):
    _env(monkeypatch, SFM_SYM=0, SFM_CUTOFF=1, SFM_REORDER=0)
    sc = _list_scene("planar")
    _recorded_tick_cell(f"ordered+boxes {name}", sc, pc.set_config(name, pc.PED_ACC), 0.05, lambda v: v.startswith("sfm_tick_kernel<"),
                        literal=False, geo=False)


# ---- sfm_fused_tick_kernel ----------------------------------------------------------------------------------------------------------
FUSED = [(name, n, z, f) for name in ("longrange", "shortrange") for n in (2, 130, 1000, 4096) for z in (0.0, 1.5) for f in ("pedacc", "all5")]
FUSED += [(name, n, z, f) for name in ("eps0", "epsneg", "lam0") for n, z, f in ((130, 0.0, "all5"), (1000, 1.5, "pedacc"), (1000, 0.0, "all5"))]


@pytest.mark.parametrize("name,n,z_spread,forces", FUSED, ids=[f"{a}-{b}-{'3d' if c else 'planar'}-{d}" for a, b, c, d in FUSED])
def test_fused_tick(name, n, z_spread, forces, monkeypatch):
    """A device-resident run(1) at dt = 1 with max_speed_factor = 1e7: the forces read back through the uncapped update
    (check_force_from_velocity, as tests/test_force_readback_gpu.py does), use_ped_radius on for the all-forces cells."""
    _env(monkeypatch, SFM_FUSED=1, SFM_CUTOFF=0)
    geo = forces == "all5"
    sc = pc.scene(n, 7000 + n, z_spread, geo=geo)
    cfg = pc.set_config(name, pc.ALL5 if geo else pc.PED_ACC, rad=geo, readback=True)
    ref = pc.Ref(sc.loc, sc.vel, sc, cfg, 1.0)
    share, amp = ref.conditions(f"fused {name} N={n}", literal=n <= 1024)
    eng = _engine(sc, cfg, 1.0, geo, boxes=True)
    try:
        eng.run(1)
        assert "fused" in eng.kernel_variant() and (("(geo)" in eng.kernel_variant()) == geo), eng.kernel_variant()
        v = eng.velocities()
    finally:
        eng.close()
    expo, absum = ref.diag["total"]
    worst, floor = P.check_force_from_velocity(f"fused {name} N={n} z={z_spread} {forces}", v, sc.vel, 1.0, ref.total, absum, expo,
                                               sc.target_speed * pc.READBACK_MSF)
    print(f"\nfused {name} N={n} z={z_spread} {forces}: exposed {share:.1%}  max_amp {amp:.3g}  worst beyond {worst:.2e}  rows on the fp32 floor {floor}")


@pytest.mark.parametrize("name", ["integrate", "integrate_fine"])
@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_fused_tick_integration_parameters(name, z_spread, monkeypatch):
    """tau 0.25, max_speed_factor 2.0, step lengths 0.1 and 0.0125 through the fused tick: v' and x' of one run(1)."""
    _env(monkeypatch, SFM_FUSED=1, SFM_CUTOFF=0)
    dt = psets.step_of(name)
    sc = pc.scene(1000, 7100, z_spread)
    sc.vel[::4] *= 3.0                                  # a quarter of the rows well above their cap of 2 x 1.2 m/s, the rest below
    cfg = pc.set_config(name, pc.ALL5, rad=True)
    ref = pc.Ref(sc.loc, sc.vel, sc, cfg, dt)
    ref.conditions(f"fused {name}")
    capped = np.linalg.norm(sc.vel + dt * ref.total, axis=1) > sc.target_speed * 2.0
    assert 20 < capped.sum() < sc.n - 20                # the cap acts on some rows and not on others
    eng = _engine(sc, cfg, dt, boxes=True)
    try:
        eng.run(1)
        assert "fused" in eng.kernel_variant(), eng.kernel_variant()
        loc, vel, _ = eng.state()
    finally:
        eng.close()
    ref.check_velocity(vel)
    x_ref = sc.loc + dt * ref.v_new
    assert np.max(np.abs(loc - x_ref)) <= 1e-6 * max(1.0, np.abs(x_ref).max()) + dt * 1e-5 * np.abs(ref.v_new).max() + dt * dt * np.nan_to_num(ref.diag["total"][0]).max()


# ---- 20 ticks re-synchronised every tick, set_params in mid-run ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_SETS)
def test_multi_tick_resync_with_set_params(name, monkeypatch):
    """tests/test_hip_parity.py::test_multi_tick_resync_and_free_run's scheme for 20 ticks under the list cutoff (carried tile boxes):
    every tick from the device's own previous fp32 state against the oracle.  After ticks 7 and 13 sfm_set_params switches to the
    other of longrange / shortrange (for those two sets: to each other and back; for the rest: to longrange and back) and the next
    tick is checked with the parameters then in force -- boxes and reach carried over from the previous epilogue included."""
    _env(monkeypatch, SFM_SYM=1, SFM_CUTOFF=1)
    n = 640
    sc = pc.scene(n, 8000)
    forces = ("acceleration_force", "pedestrian_force", "border_force", "static_obstacle_force")
    other = "shortrange" if name == "longrange" else "longrange"
    cfgs = {k: pc.set_config(k, forces, rad=True) for k in (name, other)}
    geom = O.Geometry(sc.borders, sc.border_centers, sc.border_lengths, sc.static_obstacles, [], None)
    cur = name
    eng = SfmEngine(cfgs[cur], psets.step_of(cur))
    try:
        eng.set_borders(sc.borders, sc.border_centers, sc.border_lengths)
        eng.set_static_obstacles(sc.static_obstacles)
        eng.upload_state(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, None)
        eng.set_waypoint_stream(sc.seed, sc.world_side, 2.0)
        loc, vel, wp = sc.loc.copy(), sc.vel.copy(), sc.waypoint.copy()
        draws = np.zeros(n, dtype=np.int64)
        for k in range(20):
            if k in (7, 13):
                cur = other if cur == name else name
                eng.set_params(cfgs[cur], psets.step_of(cur))
            dt = psets.step_of(cur)
            eng.run(1, redraw=True)
            assert "sym" in eng.kernel_variant(), eng.kernel_variant()
            dloc, dvel, dwp = eng.state()
            sc_k = type("S", (), dict(waypoint=wp, target_speed=sc.target_speed, radius=sc.radius))
            ref = pc.Ref(loc, vel, sc_k, cfgs[cur], dt, geom=geom)
            ref.conditions(f"resync {name} tick {k} ({cur})")
            ref.check_velocity(dvel)
            with np.errstate(all="ignore"):
                oloc, _, owp, draws = O.free_step(loc, vel, wp, sc.target_speed, sc.radius, np.zeros(n, bool), draws, geom, ref.prm, dt,
                                                  2.0, sc.seed, sc.world_side)
            assert np.max(np.abs(dloc - oloc)) <= 1e-6 * max(1.0, np.max(np.abs(oloc))) + 1e-6 + dt * dt * np.nan_to_num(ref.diag["total"][0]).max(), f"tick {k}"
            sure = np.abs(np.linalg.norm(wp[:, :2] - loc[:, :2], axis=1) - 2.0) > 1e-4
            assert np.allclose(dwp[sure], owp[sure, :2], rtol=0, atol=1e-4), f"waypoints at tick {k}"
            loc, vel = dloc, dvel
            wp = np.concatenate([dwp, np.zeros((n, 1))], axis=1)
            draws = eng.draw_counts().astype(np.int64)
    finally:
        eng.close()


# ---- the batch kernel with unlike neighbours ------------------------------------------------------------------------------------------
BATCH_SIZES = [1, 2, 64, 130, 1024, 17, 300, 65, 640, 3, 257, 96]
BATCH_SETS = ["longrange", "shortrange", "eps0", "epsneg", "lam0", "integrate"]


def _as_dict(sc):
    return vars(sc)


def _xyz(rec):
    """A batch force record's dicts name -> (N, 2 or 3) float32 as name -> (N, 3) float64."""
    def pad(a):
        out = np.zeros((len(a), 3))
        out[:, :a.shape[1]] = a
        return out
    return {("total" if k == "total" else k): pad(v) for k, v in rec.items()}


def _batch(z_spread, seed0=8500):
    scenes, cfgs, dts, names = [], [], [], []
    for k, n in enumerate(BATCH_SIZES):
        name = BATCH_SETS[k % len(BATCH_SETS)]
        scenes.append(pc.scene(n, seed0 + k, z_spread))
        cfgs.append(pc.set_config(name, pc.ALL5, rad=bool(k % 2)))
        dts.append(psets.step_of(name))
        names.append(name)
    return scenes, cfgs, dts, names


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_batch_tick_forces_with_unlike_neighbours(z_spread):
    """Twelve scenes of mixed sizes, consecutive scenes on different parameter sets: tick_forces force by force and v'."""
    scenes, cfgs, dts, names = _batch(z_spread)
    b = SfmBatch(cfgs, dts)
    try:
        b.upload([_as_dict(s) for s in scenes])
        rec = b.tick_forces()
        states = b.state()
    finally:
        b.close()
    exposed = rows = 0
    for k, (sc, cfg, dt) in enumerate(zip(scenes, cfgs, dts)):
        ref = pc.Ref(sc.loc, sc.vel, sc, cfg, dt)
        assert ref.max_amp <= pc.MAX_AMP, (k, ref.max_amp)
        exposed, rows = exposed + ref.exposed, rows + sc.n
        worst = ref.check_forces(f"batch scene {k} ({names[k]}, N={sc.n})", lambda nm, r=_xyz(rec[k]): r[nm])
        vw = ref.check_velocity(states[k][1])
        print(f"\nbatch scene {k} {names[k]} N={sc.n}: exposed {ref.share:.1%}  max_amp {ref.max_amp:.3g}  worst {worst:.2e}  v' rel {vw:.2e}")
    # the cell is the batch (one row of a 3-pedestrian scene is a third of it): exposed rows over all rows
    assert exposed <= pc.MAX_EXPOSED_SHARE * rows, (exposed, rows)


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_batch_ten_ticks_resynchronised(z_spread):
    """10 integrating ticks, every tick from the device's own fp32 state against the oracle; device-side vehicles (moved by the
    kernel, followed here by the host twin scenarios.advance_dynamic) in every scene that has vehicles."""
    import copy
    scenes, cfgs, dts, names = _batch(z_spread, 8600)
    scenes = [copy.deepcopy(s) for s in scenes]
    assert sum(len(s.dynamic_obstacles) > 0 for s in scenes) >= 2
    b = SfmBatch(cfgs, dts)
    try:
        b.upload([_as_dict(s) for s in scenes], device_vehicles=True)
        cur = [(np.float32(s.loc).astype(np.float64), np.float32(s.vel).astype(np.float64)) for s in scenes]
        exposed = rows = 0
        for t in range(10):
            b.tick(integrate=True)
            got = b.state()
            for k, (sc, cfg, dt) in enumerate(zip(scenes, cfgs, dts)):
                loc, vel = cur[k]
                ref = pc.Ref(loc, vel, sc, cfg, dt)
                assert ref.max_amp <= pc.MAX_AMP, (k, t, ref.max_amp)
                exposed, rows = exposed + ref.exposed, rows + sc.n
                dloc, dvel = got[k]
                ref.check_velocity(dvel)
                x_ref = loc + dt * ref.v_new
                assert np.max(np.abs(dloc - x_ref)) <= 1e-6 * max(1.0, np.abs(x_ref).max()) + 1e-6 + dt * dt * np.nan_to_num(ref.diag["total"][0]).max(), (k, t)
                cur[k] = (dloc, dvel)
                scenarios.advance_dynamic(sc, dt)
        assert exposed <= pc.MAX_EXPOSED_SHARE * rows, (exposed, rows)     # (over the whole batch and all ten ticks)
    finally:
        b.close()


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_batch_scene_is_independent_of_its_neighbours_parameters(z_spread):
    """The same scene with the same parameters, bit for bit, whichever parameter sets its neighbours carry: the neighbours differ
    in parameters ONLY (same crowds, same geometry)."""
    target = pc.scene(130, 8700, z_spread)
    tcfg = pc.set_config("epsneg", pc.ALL5, rad=True)
    others = [pc.scene(n, 8710 + k, z_spread) for k, n in enumerate((64, 257, 1, 640))]
    out = []
    for neighbours in (("stock",) * 4, ("longrange", "shortrange", "lam0", "eps0"), ("shortrange", "longrange", "eps0", "lam0")):
        cfgs = [pc.set_config(nm, pc.ALL5, rad=True) for nm in neighbours]
        b = SfmBatch(cfgs[:2] + [tcfg] + cfgs[2:], [0.05] * 5)
        try:
            b.upload([_as_dict(s) for s in others[:2] + [target] + others[2:]])
            rec = b.tick_forces()
            out.append((_xyz(rec[2]), b.state()[2]))
        finally:
            b.close()
    for rec, (loc, vel) in out[1:]:
        for nm in out[0][0]:
            assert np.array_equal(rec[nm], out[0][0][nm], equal_nan=True), nm
        assert np.array_equal(vel, out[0][1][1], equal_nan=True) and np.array_equal(loc, out[0][1][0], equal_nan=True)


# ---- parameters at the edges the ABI lets through, and the ones it refuses ------------------------------------------
EDGES = {"msf0": {"max_speed_factor": 0.0}, "msf_negative": {"max_speed_factor": -0.5}, "tiny_step": {}, "huge_tau": {"goal_force": {"tau": 1e6}},
         "lambda_negative": {}}


@pytest.mark.parametrize("edge", list(EDGES))
def test_edge_parameters_match_the_oracle(edge, monkeypatch):
    """What check_params lets through is computed like the reference computes it: a speed cap of 0 (v' = 0) or below 0 (np.minimum(1,
    max_speed / speed) < 0 turns v' round, stateutils.py:18-23), a step length of 1e-4, tau = 1e6, and a negative lambda -- for
    which the tile cutoff switches itself off (its reach assumes lambda >= 0): the tick falls back to the full pair grid, silently,
    as INTEGRATION.md states."""
    _env(monkeypatch, SFM_SYM=1, SFM_CUTOFF=1, SFM_REORDER=0)
    sc = pc.scene(1000, 9000)
    cfg = pc.set_config("stock", pc.ALL5, rad=True)
    cfg.update(EDGES[edge])
    dt = 1e-4 if edge == "tiny_step" else 0.05
    if edge == "lambda_negative":
        cfg["pedestrian_force"]["lambda"] = -0.5
    work = _recorded_tick_cell(f"edge {edge}", sc, cfg, dt, lambda v: "sym" in v)
    n_t = (sc.n + 63) // 64
    if edge == "lambda_negative":
        assert work[0] == n_t * (n_t - 1) // 2 + (n_t + 1) // 2      # no list: every tile pair


def test_refused_parameters_leave_the_handle_and_the_batch_usable():
    """gamma <= 0 of an enabled Moussaid force, b <= 0 of the border force, a non-finite tau / step length / speed factor: refused by
    sfm_create, sfm_set_params and sfm_batch_set_params with a message that names the parameter; the handle keeps its parameters."""
    lib = _lib.load()
    sc = pc.scene(300, 9100)
    cfg = pc.set_config("longrange", pc.ALL5)
    ref = pc.Ref(sc.loc, sc.vel, sc, cfg, 0.05)
    eng = _engine(sc, cfg, 0.05)
    try:
        for mutate, word in ((lambda p: setattr(p.pedestrian, "gamma", -0.35), "pedestrian_force.gamma"),
                             (lambda p: setattr(p, "border_b", -0.3), "border_force.b"),
                             (lambda p: setattr(p.static_obstacle, "gamma", 0.0), "static_obstacle_force.gamma"),
                             (lambda p: setattr(p.dynamic_obstacle, "gamma", float("nan")), "dynamic_obstacle_force.gamma"),
                             (lambda p: setattr(p, "tau", float("inf")), "tau"),
                             (lambda p: setattr(p, "max_speed_factor", float("nan")), "max_speed_factor"),
                             (lambda p: setattr(p, "step_length", float("inf")), "step_length")):
            bad = params_from_config(cfg, 0.05)
            mutate(bad)
            assert lib.sfm_set_params(eng._h, C.byref(bad)) == -1 and word in lib.sfm_last_error(eng._h).decode(), word
            h = C.c_void_p()
            assert lib.sfm_create(C.byref(bad), 0, C.byref(h)) == -1 and word in lib.sfm_last_error(None).decode(), word
        eng.tick(record=True)                            # ... and the handle still runs, with the parameters it had
        ref.check_forces("after refusals", eng.forces)
    finally:
        eng.close()
    b = SfmBatch([cfg, cfg], [0.05, 0.05])
    try:
        b.upload([_as_dict(sc), _as_dict(pc.scene(64, 9101))])
        prm = batch_params([cfg, cfg], [0.05, 0.05])
        prm[1].border_b = -0.3
        assert lib.sfm_batch_set_params(b._b, prm) != 0
        msg = lib.sfm_batch_last_error(b._b).decode()
        assert "scene 1" in msg and "border_force.b" in msg, msg
        rec = b.tick_forces()
        ref.check_forces("batch after a refusal", lambda nm, r=_xyz(rec[0]): r[nm])
    finally:
        b.close()
