"""Nearest-point choice and culls AT EXACT TIES on every geometry path of the device (tests/_geo_cases.py says what the cases are,
tests/test_geo_cases_host.py that the oracle alone makes them meaningful).  Run with  python -m pytest tests/test_geo_cases_gpu.py -m gpu -s.

One rule everywhere: ``P.check_force`` unchanged (1e-5 relative, ATOL 1e-9) with NO allowance for a tie or a cull -- the inputs are
exact in fp32, so the device's comparisons are the exact comparisons and np.argmin's first-minimum rule and the strict ``<`` of the
culls (forces.py:149-155, 222-229) are asserted themselves.  Each geometry force is checked on its own, then the total; what is exact
is compared bit for bit (a dropped polyline's 0, the 0 of a pedestrian standing on a border point, the z component, a 3-D crowd
against the planar one, the straight-border shortcut against the full scan, the observations' floats).  Every test prints the worst
error / allowance it saw.

Paths: the handle's geometry kernel in the two-launch tick (ordered and symmetric, inside the pair launch and alone, 1 slice and the
default, shortcut on and off; the finder's list overflow), the geometry role of the fused tick, the host-in-the-loop step, the force
classes of ``forces.py``, the batch tick with given and with device-side vehicles, and the observations.

The fused tick cannot record its forces.  Its force is read back through one uncapped update at dt = 64 (a power of two: dt F is
exact) with max_speed_factor 1e7: F = (v' - v) / dt carries the one rounding of v', 2^-24 |v + 64 F| / 64 <= 2^-24 (|v| / 64 + |F|).
With |v| <= 4 m/s and kept terms >= 1e-3 m/s^2 that is below 4e-9 + 6e-8 |F|, inside check_force's 1e-9 + 1e-5 |F| at every term
size, so the plain check_force holds the read-back too; a dropped row's v' is v bit for bit.
"""
import types

import numpy as np
import pytest

import _geo_cases as G
import _parity as P
from carla_social_force_model_amd import forces as hip_forces
from carla_social_force_model_amd.batch import OBS_HEADER, SfmBatch
from carla_social_force_model_amd.engine import SfmEngine
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

KNOBS = ("SFM_SYM", "SFM_IPW", "SFM_TEAM", "SFM_CUTOFF", "SFM_REORDER", "SFM_FUSED", "SFM_PAIR_GEO", "SFM_GEO_SLICES", "SFM_NO_STRAIGHT",
         "SFM_POOL", "SFM_STRIPS", "SFM_RESORT_EVERY")
NAMES = G.FORCE_OF_KIND + ("total",)
DT = 0.05
READBACK_DT, READBACK_MSF = 64.0, 1e7
_REF = {}


def _env(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))


def _ref(c, rad):
    key = (id(c), bool(rad))
    if key not in _REF:
        _REF[key] = (c, G.reference(c, G.config(rad)))          # (the crowd is kept alive with its reference: ids are not reused)
    return _REF[key][1]


def _pad3(a):
    out = np.zeros((len(a), 3))
    out[:, :a.shape[1]] = a
    return out


def _verdict(label, c, ref, get, names=NAMES):
    """check_force with exposure identically 0 on every named force, then what is exact, bit for bit.  Returns worst err / allowance."""
    zero, worst = np.zeros(c.n), 0.0
    kept = G.kept(c)
    for name in names:
        got = np.asarray(get(name), dtype=np.float64)
        want = ref.total if name == "total" else ref.per[name]
        absum = ref.diag[name][1]
        P.check_force(f"{label} {name}", got, want, absum, zero)
        allow = P.RTOL * np.maximum(np.linalg.norm(want, axis=1), np.nan_to_num(absum)) + P.ATOL
        worst = max(worst, float(np.max(np.linalg.norm(got - want, axis=1) / allow)))
        assert not got[:, 2].any(), f"{label} {name}: a z component"
        off = ~kept.any(axis=1) if name == "total" else ~kept[:, G.FORCE_OF_KIND.index(name)]
        assert not got[off].any(), f"{label} {name}: a dropped polyline left a force on rows {np.flatnonzero(got[off].any(axis=1))[:5]}"
        if name == "border_force":
            on = np.array([cs.zero_term for cs in c.cases])
            assert not got[on].any(), f"{label}: a pedestrian on a border point"
    return worst


def _engine(c, cfg, dt=DT):
    eng = SfmEngine(cfg, dt)
    try:
        eng.set_borders(c.borders, c.border_centers, c.border_lengths)
        eng.set_static_obstacles(c.static_obstacles)
        eng.set_dynamic_obstacles(c.dynamic_obstacles, c.dynamic_vel)
        eng.upload_state(c.loc, c.vel, c.waypoint, c.target_speed, c.radius, None)
    except Exception:
        eng.close()
        raise
    return eng


def _recorded(c, rad, expect):
    """One recorded two-launch tick: name -> (n, 3) of the three geometry forces, the pedestrian force and the total."""
    eng = _engine(c, G.config(rad))
    try:
        assert eng.planar == (not c.loc[:, 2].any())
        eng.tick(record=True)
        assert expect(eng.kernel_variant()), eng.kernel_variant()
        out = {name: eng.forces(name) for name in NAMES + ("pedestrian_force",)}
        loc, _, _ = eng.state()
    finally:
        eng.close()
    assert np.array_equal(loc[:, :2], c.loc[:, :2])                # caller order
    assert not np.nan_to_num(out["pedestrian_force"]).any() and not np.isnan(out["pedestrian_force"]).any()
    return out


def _expect(n):
    return (lambda v: v.startswith("sfm_tick_kernel<")) if n < 256 else (lambda v: "sym" in v)


# ---- the handle's geometry kernel, two-launch tick --------------------------------------------------------------------------------------
HANDLE = [(n, pg, sl, ns) for n in (65, 320) for pg in (0, 1) for sl in (1, None) for ns in (False, True)]


@pytest.mark.parametrize("n,pair_geo,slices,no_straight", HANDLE,
                         ids=[f"N{n}-pairgeo{pg}-slices{sl or 'default'}-{'scan' if ns else 'shortcut'}" for n, pg, sl, ns in HANDLE])
def test_two_launch_tick(n, pair_geo, slices, no_straight, monkeypatch):
    """N = 65: the ordered kernel; N = 320: the symmetric pair kernel.  Geometry workgroups inside the pair launch (SFM_PAIR_GEO=1) or in
    a launch of their own, one slice per tile or the default four, the straight-border shortcut on or off."""
    _env(monkeypatch, SFM_FUSED=0, SFM_CUTOFF=0, SFM_PAIR_GEO=pair_geo, SFM_GEO_SLICES=slices, SFM_NO_STRAIGHT=1 if no_straight else None)
    crowds = G.covering_crowds(n)
    assert G.covered(crowds)
    worst = 0.0
    for q, c in enumerate(crowds):
        got = _recorded(c, False, _expect(n))
        worst = max(worst, _verdict(f"two-launch N={n} crowd {q}", c, _ref(c, False), got.__getitem__))
    print(f"\ntwo-launch N={n} pair_geo={pair_geo} slices={slices} no_straight={no_straight}: worst err / allowance {worst:.3f}")


@pytest.mark.parametrize("n", [65, 320])
@pytest.mark.parametrize("rad,z3", [(True, False), (False, True), (True, True)], ids=["radius", "3d", "3d-radius"])
def test_two_launch_tick_with_radius_and_in_3d(rad, z3, n, monkeypatch):
    """use_ped_radius at radius 0.25, and a 3-D crowd (dyadic z and v_z) -- which must give the planar crowd's geometry forces, bit for bit."""
    worst = 0.0
    for env in (dict(SFM_FUSED=0, SFM_CUTOFF=0), dict(SFM_FUSED=0, SFM_CUTOFF=0, SFM_PAIR_GEO=0, SFM_GEO_SLICES=1)):
        _env(monkeypatch, **env)
        for q, c in enumerate(G.covering_crowds(n, z3)):
            got = _recorded(c, rad, _expect(n))
            worst = max(worst, _verdict(f"two-launch N={n} rad={rad} 3d={z3} crowd {q}", c, _ref(c, rad), got.__getitem__))
            if z3:
                flat = _recorded(G.covering_crowds(n, False)[q], rad, _expect(n))
                for name in NAMES:
                    assert np.array_equal(got[name], flat[name]), f"{name}: the 3-D crowd's force is not the planar crowd's"
    print(f"\ntwo-launch N={n} rad={rad} 3d={z3}: worst err / allowance {worst:.3f}")


def test_the_shortcut_and_the_scan_pick_the_same_points(monkeypatch):
    """The straight cases through geo_item's five-sample window and through lane_nearest's full scan: the same point, so the same
    arithmetic and the same bits -- and the oracle's point (the verdict)."""
    c = G.covering_crowds(320)[0]
    straight = np.array(["straight" in cs.tags for cs in c.cases])
    assert straight.sum() == 48
    out = []
    for ns in (None, 1):
        _env(monkeypatch, SFM_FUSED=0, SFM_CUTOFF=0, SFM_NO_STRAIGHT=ns)
        out.append(_recorded(c, False, _expect(320)))
        worst = _verdict(f"no_straight={ns}", c, _ref(c, False), out[-1].__getitem__)
    for name in NAMES:
        assert np.array_equal(out[0][name], out[1][name]), name
    print(f"\nshortcut against scan: 48 straight rows bit for bit, worst err / allowance {worst:.3f}")


# ---- the finder's on-the-spot scan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair_geo", [0, 1])
@pytest.mark.parametrize("per_kind", G.MULTI_KINDS, ids=["3+3+3", "9-borders", "9-static"])
def test_finder_list_overflow(per_kind, pair_geo, monkeypatch):
    """64 rows (one tile), 9 kept polylines each, one slice: each of the 16 waves keeps 36, its list holds GEO_ITEMS = 32, the rest
    is scanned on the spot by the finder's second pass.  The count is made on the host (``G.finder_positions`` restates the deal)."""
    _env(monkeypatch, SFM_FUSED=0, SFM_CUTOFF=0, SFM_REORDER=0, SFM_PAIR_GEO=pair_geo, SFM_GEO_SLICES=1)
    c = G.multi_crowd(64, per_kind, "random", 3 + G.MULTI_KINDS.index(per_kind))
    pos = np.concatenate([p for p in G.finder_positions(c, 1) if len(p)])
    assert (pos[:, 2] >= 0).all() and len(pos) == 64 * 9
    per_wave = np.bincount(pos[:, 1], minlength=G.GEO_WAVES)
    assert (per_wave > G.GEO_ITEMS).all(), per_wave                   # every wave overflows its list
    above = pos[:, 2] >= G.GEO_ITEMS
    assert above.sum() == 64 and (~above).sum() == 512                # designed polylines below and above the capacity
    by_kind = [p[:, 2] >= G.GEO_ITEMS for p in G.finder_positions(c, 1)]
    last = max(k for k in range(3) if per_kind[k])
    assert by_kind[last].sum() == 64 and any((~b).any() for b in by_kind if len(b))
    got = _recorded(c, False, _expect(64))
    worst = _verdict(f"overflow {per_kind}", c, _ref(c, False), got.__getitem__)
    print(f"\nfinder overflow {per_kind} pair_geo={pair_geo}: {per_wave.max()} kept per wave, worst err / allowance {worst:.3f}")


# ---- the fused tick's geometry role -----------------------------------------------------------------------------------------------------
def _family_config(family, rad):
    cfg = G.config(rad, READBACK_MSF)
    if family != "total":
        for name in G.FORCE_OF_KIND:
            cfg["forces"][name] = name == family
    return cfg


@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
@pytest.mark.parametrize("n", [64, 320])
def test_fused_tick_geometry_role(n, z3, monkeypatch):
    """sfm_run(1) on sfm_fused_tick_kernel(geo), one geometry family at a time and all three (see the module docstring for the
    read-back).  use_ped_radius on in the 3-D cells."""
    _env(monkeypatch, SFM_FUSED=1, SFM_CUTOFF=0)
    rad, worst = z3, 0.0
    for q, c in enumerate(G.covering_crowds(n, z3)):
        assert np.abs(c.vel).max() <= 4.0
        got = {}
        for family in NAMES:
            eng = _engine(c, _family_config(family, rad), READBACK_DT)
            try:
                eng.run(1)
                kinds = range(3) if family == "total" else (G.FORCE_OF_KIND.index(family),)
                geo = any(len(c.owner[k]) for k in kinds)      # (a crowd without a polyline of the family: no geometry workgroups)
                assert eng.kernel_variant() == ("sfm_fused_tick_kernel(geo)" if geo else "sfm_fused_tick_kernel"), eng.kernel_variant()
                v = eng.velocities()
            finally:
                eng.close()
            got[family] = (v - c.vel) / READBACK_DT
        worst = max(worst, _verdict(f"fused N={n} 3d={z3} crowd {q}", c, _ref(c, rad), got.__getitem__))
    print(f"\nfused tick geometry role N={n} 3d={z3}: worst err / allowance {worst:.3f}")


# ---- the host-in-the-loop step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rad,z3", [(False, False), (True, False), (False, True)], ids=["plain", "radius", "3d"])
def test_step_packed(rad, z3):
    worst, n_still = 0.0, 0
    cfg = G.config(rad)
    for c in G.covering_crowds(65, z3):
        ref = _ref(c, rad)
        rows = np.zeros((c.n, 9), np.float32)
        rows[:, 0:2], rows[:, 2:4], rows[:, 4:6] = c.loc[:, :2], c.vel[:, :2], c.waypoint[:, :2]
        rows[:, 6], rows[:, 7] = c.target_speed, c.radius
        zvz = np.ascontiguousarray(np.stack([c.loc[:, 2], c.vel[:, 2]], axis=1), dtype=np.float32) if z3 else None
        v = np.full((c.n, 3), np.nan, np.float32)
        eng = SfmEngine(cfg, DT)
        try:
            eng.set_borders(c.borders, c.border_centers, c.border_lengths)
            eng.set_static_obstacles(c.static_obstacles)
            eng.set_dynamic_obstacles(c.dynamic_obstacles, c.dynamic_vel)
            eng.step_packed(rows, zvz, v)
        finally:
            eng.close()
        v_ref = O.new_velocities(c.vel, ref.total, c.target_speed, DT)
        worst = max(worst, P.check_velocity(v, v_ref, np.zeros(c.n), DT))
        still = ~G.kept(c).any(axis=1) & (np.linalg.norm(c.vel, axis=1) <= c.target_speed * 1.3)
        assert np.array_equal(v[still].astype(np.float64), c.vel[still])                      # no force, no cap: v' is v
        n_still += int(still.sum())
    assert n_still >= 2
    print(f"\nstep_packed rad={rad} 3d={z3}: worst |dv'| / |v'| {worst:.2e} (bound 1e-5)")


# ---- the force classes ------------------------------------------------------------------------------------------------------------------
class _Peds:
    """What ``forces._columns`` reads of a PedState."""

    def __init__(self, c):
        st = np.zeros(c.n, dtype=[("loc", "f8", 3), ("vel", "f8", 3), ("next_waypoint", "f8", 3), ("target_speed", "f8"), ("radius", "f8"),
                                  ("mode", "O")])
        st["loc"], st["vel"], st["next_waypoint"], st["target_speed"], st["radius"] = c.loc, c.vel, c.waypoint, c.target_speed, c.radius
        st["mode"] = [types.SimpleNamespace(current_mode=1) for _ in range(c.n)]
        self.state = st

    def size(self):
        return len(self.state)


def test_force_classes(monkeypatch):
    """BorderForce / ObstacleForce of ``forces.py``, each on a handle of its own with only its force on."""
    _env(monkeypatch)
    c = G.covering_crowds(320)[0]
    cfg = G.config(False)
    info = [[c.border_centers[k], float(c.border_lengths[k])] for k in range(len(c.borders))]
    fs = {"border_force": hip_forces.BorderForce(DT, cfg, c.borders, info),
          "static_obstacle_force": hip_forces.ObstacleForce(DT, cfg),
          "dynamic_obstacle_force": hip_forces.ObstacleForce(DT, cfg, True)}
    try:
        fs["static_obstacle_force"].update_obstacles(c.static_obstacles)
        fs["dynamic_obstacle_force"].update_obstacles(c.dynamic_obstacles)
        fs["dynamic_obstacle_force"].update_obstacle_velocities(c.dynamic_vel)
        peds = _Peds(c)
        got = {name: f.get_force(peds) for name, f in fs.items()}
    finally:
        for f in fs.values():
            f.close()
    worst = _verdict("force classes", c, _ref(c, False), got.__getitem__, G.FORCE_OF_KIND)
    print(f"\nforce classes: worst err / allowance {worst:.3f}")


# ---- the batch tick ---------------------------------------------------------------------------------------------------------------------
def _boxes(crowds):
    """The scenes' vehicles for sfm_batch_set_dynamic_boxes with the DESIGNED rings: local offsets ring - centre at yaw 0, so the
    device forms centre + offset, the uploaded point, exactly."""
    item_off, off, u, ctr, vel = [0], [0], [], [], []
    for c in crowds:
        for (cen, ring), v in zip(c.dynamic_obstacles, c.dynamic_vel):
            u.append(ring - cen)
            ctr.append(cen)
            vel.append(v)
            off.append(off[-1] + len(ring))
        item_off.append(item_off[-1] + len(c.dynamic_obstacles))
    u, ctr, vel = np.concatenate(u), np.array(ctr), np.array(vel)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    M = len(ctr)
    return (np.array(item_off, np.int32), np.array(off, np.int32), f32(u[:, 0]), f32(u[:, 1]), f32(ctr[:, 0]), f32(ctr[:, 1]),
            np.ones(M, np.float32), np.zeros(M, np.float32), f32(vel[:, 0]), f32(vel[:, 1]))


@pytest.mark.parametrize("device_vehicles", [False, True], ids=["given-rings", "device-vehicles"])
@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
def test_batch_tick(z3, device_vehicles):
    """Scenes of 3, 64, 65, 128, 130 and 300 rows in one batch (the 4 / 2 / 1 j-slice forms, one and two passes), use_ped_radius in
    every other scene; ``tick_forces(integrate=False)``.  With device-side vehicles the ring of the tick is the uploaded one."""
    crowds = G.scene_crowds(G.BATCH_SIZES, z3)
    assert G.covered(crowds)
    rads = [bool(q % 2) for q in range(len(crowds))]
    b = SfmBatch([G.config(r) for r in rads], [DT] * len(crowds))
    try:
        b.upload([c.scene() for c in crowds])
        if device_vehicles:
            b.set_dynamic_boxes(_boxes(crowds))
            for c, veh in zip(crowds, b.dynamic_obstacles()):
                for (cen, ring), (dcen, dring) in zip(c.dynamic_obstacles, veh):
                    assert np.array_equal(cen, dcen) and np.array_equal(ring, dring), "the device's ring is not the designed one"
        assert b.planar == (not z3)
        rec = b.tick_forces(integrate=False)
        states = b.state()
    finally:
        b.close()
    worst = 0.0
    for q, (c, rad) in enumerate(zip(crowds, rads)):
        assert np.array_equal(states[q][0][:, :2], c.loc[:, :2])       # caller order, nothing moved
        assert rec[q]["total"].shape == (c.n, 3 if z3 else 2)
        assert not rec[q]["pedestrian_force"].any()
        worst = max(worst, _verdict(f"batch scene {q} (N={c.n}, rad={rad})", c, _ref(c, rad), lambda name: _pad3(rec[q][name])))
    if z3:                                                             # the planar batch's geometry forces, bit for bit
        flat = G.scene_crowds(G.BATCH_SIZES, False)
        b = SfmBatch([G.config(r) for r in rads], [DT] * len(flat))
        try:
            b.upload([c.scene() for c in flat])
            if device_vehicles:
                b.set_dynamic_boxes(_boxes(flat))
            rec0 = b.tick_forces(integrate=False)
        finally:
            b.close()
        for q in range(len(flat)):
            for name in NAMES:
                assert np.array_equal(rec[q][name][:, :2], rec0[q][name]), (q, name)
    print(f"\nbatch tick 3d={z3} device_vehicles={device_vehicles}: worst err / allowance {worst:.3f}")


# ---- observations -----------------------------------------------------------------------------------------------------------------------
def _brute_force(c, sense_range):
    """The contract of include/sfm_hip.h in float64: per kind the first minimum of d2 = (x - px)^2 + (y - py)^2 over ALL points of ALL
    the scene's polylines in CSR order; present iff d2 < R^2.  Every d2 is exact in float64 (multiples of 1/256 below 2^27).
    Returns (floats 8-15 (n, 8), flags (n,))."""
    out, flags = np.zeros((c.n, 8)), np.zeros(c.n)
    x = c.loc[:, :2]
    for kind, col, bit in ((2, 0, 4.0), (0, 4, 1.0), (1, 6, 2.0)):
        K = len(c.owner[kind])
        if K == 0:
            continue
        pts = np.concatenate([c.points(kind, k) for k in range(K)])
        which = np.concatenate([np.full(len(c.points(kind, k)), k) for k in range(K)])
        d = x[:, None, :] - pts[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        idx = np.argmin(d2, axis=1)
        present = d2[np.arange(c.n), idx] < sense_range * sense_range
        out[:, col:col + 2] = np.where(present[:, None], pts[idx] - x, 0.0)
        if kind == 2:
            out[:, 2:4] = np.where(present[:, None], c.dynamic_vel[which[idx]] - c.vel[:, :2], 0.0)
        flags += bit * present
    return out, flags


@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
def test_observations(z3):
    """Frame 0, K = 4: scenes of 40 rows (the role-split form) and 65 and 300 rows (a wave per 64 rows) at a range of 16 m, and the
    65-row scene again at a range of EXACTLY 1.25 m, where a point of the tie material (d2 = 25/16 = R^2) is absent by the strict <
    and a point one quantum nearer is present."""
    crowds = G.scene_crowds(G.OBSERVE_SIZES, z3, seed=40)
    crowds.append(crowds[1])
    ranges = [16.0, 16.0, 16.0, 1.25]
    b = SfmBatch(G.config(False), DT, B=len(crowds))
    try:
        b.upload([c.scene() for c in crowds])
        b.set_observation(4, ranges, 0)
        got = b.observations()
    finally:
        b.close()
    cross = 0
    for q, (c, R, rec) in enumerate(zip(crowds, ranges, got)):
        assert rec.dtype == np.float32 and rec.shape == (c.n, OBS_HEADER + 16)
        want, flags = _brute_force(c, R)
        assert np.array_equal(rec[:, 8:16].astype(np.float64), want), f"scene {q}: rows {np.flatnonzero((rec[:, 8:16] != want).any(axis=1))[:5]}"
        assert np.array_equal(rec[:, 7].astype(np.float64), flags), f"scene {q}: flags"
        assert np.array_equal(rec[:, 0:2].astype(np.float64), c.waypoint[:, :2] - c.loc[:, :2])
        assert np.array_equal(rec[:, 2:4].astype(np.float64), c.vel[:, :2]) and (rec[:, 5] == 1.0).all()
        assert not rec[:, 6].any() and not rec[:, OBS_HEADER:].any()           # nobody within 16 m
        # the designed expectation: the row's own polylines, the lower index among equally near points, in or out of range by d2 < R^2
        pt, item, d2 = G.expected_points(c)
        has = (item >= 0) & (d2 < R * R)
        assert np.array_equal(flags, has[:, 0] * 1.0 + has[:, 1] * 2.0 + has[:, 2] * 4.0), f"scene {q}: designed flags"
        for kind, col in ((2, 0), (0, 4), (1, 6)):
            assert np.array_equal(want[:, col:col + 2], np.where(has[:, kind, None], pt[:, kind] - c.loc[:, :2], 0.0)), (q, kind)
        rows = np.flatnonzero(has[:, 2])
        assert np.array_equal(want[rows, 2:4], c.dynamic_vel[item[rows, 2]] - c.vel[rows, :2])
        if R == 1.25:
            at = (item >= 0) & (d2 == G.TIE_D2)
            assert at.any() and not has[at].any() and has.any()                 # both sides of the strict <
        for r, cs in enumerate(c.cases):                                        # the cross-polyline rule
            if "cross" in cs.tags and R == 16.0:
                kind = cs.polys[0].kind
                mine = np.flatnonzero(c.owner[kind] == r)
                assert len(mine) == 2 and item[r, kind] == mine.min()
                cross += 1
    assert cross >= 3
    print(f"\nobservations 3d={z3}: {sum(c.n for c in crowds)} rows bit for bit, {cross} cross-polyline rows")
