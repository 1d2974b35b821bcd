"""The per-pedestrian tick update AT EXACT TIES on every kernel path of the device (tests/_update_cases.py says what the rows are,
tests/test_update_cases_host.py that the oracle alone makes them meaningful).  Run with
python -m pytest tests/test_update_cases_gpu.py -m gpu -s.

One verdict everywhere (``_verdict``), with no exemption and no exposure:
  decisions   the arrived set, the draw counters, the redrawn waypoints (bitwise the oracle's fp32 draw, keyed by the caller's index)
              and the untouched ones (bitwise), with redraw off nothing changes at all;
  exact rows  v' = 0 and x' = x where the case says so, on every path; the designed v' bit for bit (the velocity returned unchanged
              at the exact cap, the halved one, v / 2, ts e) on the IEEE paths;
  the rest    ``P.check_velocity`` unchanged (1e-5 per pedestrian) against ``O.new_velocities`` in float64; the worst distance of v'
              from the oracle in fp32 units in the last place of the row's largest component is printed;
  x'          the correctly rounded fp32 fma(dt, v'_device, x), formed in rational arithmetic, component by component and bit for
              bit; x itself with integrate off.
Each cell asserts the path it ran and runs twice: with the acceleration force alone (on the paths that only run with the pedestrian
force switched on: with A = 0) and with the stock pedestrian force, which the lattice makes exactly 0 -- the two outcomes must be
the same numbers.
"""
import numpy as np
import pytest

import _parity as P
import _update_cases as U
from carla_social_force_model_amd.batch import SfmBatch
from carla_social_force_model_amd.engine import SfmEngine
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

KNOBS = ("SFM_SYM", "SFM_IPW", "SFM_TEAM", "SFM_CUTOFF", "SFM_REORDER", "SFM_FUSED", "SFM_FUSED_LEAN", "SFM_PAIR_GEO", "SFM_GEO_SLICES",
         "SFM_NO_STRAIGHT", "SFM_POOL", "SFM_STRIPS", "SFM_RESORT_EVERY")
LEAN, GENERAL = "sfm_fused_tick_kernel<lean>", "sfm_fused_tick_kernel<general>"
SYM = "sfm_pair_sym_kernel+sfm_sym_epilogue_kernel"
FLAGS = [(True, True), (True, False), (False, True), (False, False)]          # (integrate, redraw)
SETS = [(pset, thr) for pset in U.PSETS for thr in U.THRESHOLDS]


def _env(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))


def _row_ulp(got, ref):
    """Worst |got - fp32(ref)| in units in the last place of each row's largest |component|."""
    ref32 = np.float32(ref).astype(np.float64)
    top = np.abs(ref32).max(axis=1)
    ok = top > 0
    if not ok.any():
        return 0.0
    scale = np.spacing(np.float32(top[ok])).astype(np.float64)
    return float(np.max(np.abs(np.asarray(got)[ok] - ref32[ok]).max(axis=1) / scale))


def _flat(cr, loc, vel):
    """A planar crowd's downloads as (n, 3) with z = v_z = 0."""
    loc, vel = np.array(loc, dtype=np.float64), np.array(vel, dtype=np.float64)
    if not cr.z3:
        assert not np.nan_to_num(vel[:, 2]).any()
        loc[:, 2], vel[:, 2] = 0.0, 0.0
    return loc, vel


def _verdict(label, cr, snap, integrate, redraw, ieee, e=None, skip=None):
    """See the module docstring.  ``snap`` = (loc, vel, waypoint (n, 2), draws); ``skip``: rows the path parks.  Returns (worst
    |dv'| / |v'|, worst row ulp)."""
    loc, vel, wp, draws = snap
    loc, vel = _flat(cr, loc, vel)
    e = U.expectation(cr) if e is None else e
    keep = np.ones(cr.n, bool) if skip is None else ~skip
    names = lambda m: [f"{r}:{cr.cases[r].name}" for r in np.flatnonzero(m)[:6]]
    assert np.array_equal(e.arrived, cr.arrived)
    if draws is not None:
        want_d = e.draws if redraw else np.zeros(cr.n, np.int64)
        assert np.array_equal(np.asarray(draws, dtype=np.int64), want_d), f"{label}: arrived set / counters {names(draws != want_d)}"
    want_wp = e.waypoint if redraw else cr.waypoint[:, :2]
    bad = (np.asarray(wp, dtype=np.float64) != want_wp).any(axis=1)
    assert not bad.any(), f"{label}: waypoints {names(bad)}"
    z = cr.zero & keep
    assert not vel[z].any(), f"{label}: v' = 0 rows {names(z & vel.any(axis=1))}"
    assert np.array_equal(loc[z], cr.loc[z]), f"{label}: x' = x rows"
    if ieee:
        rows, vals = cr.v_exact()
        bad = np.zeros(cr.n, bool)
        bad[rows] = (vel[rows] != vals).any(axis=1)
        bad &= keep
        assert not bad.any(), f"{label}: exact v' {names(bad)}: {vel[bad][:3]}"
    worst = P.check_velocity(vel[keep], e.v[keep], np.zeros(int(keep.sum())), cr.dt)
    x_want = U.fma_f32(cr.dt, vel, cr.loc) if integrate else cr.loc
    bad = (loc != x_want).any(axis=1) & keep
    assert not bad.any(), f"{label}: x' is not fma(dt, v', x) on {names(bad)}"
    return worst, _row_ulp(vel[keep], e.v[keep])


def _engine(cr, ped, rad=False, border=False):
    eng = SfmEngine(U.config(cr.pset, ped, rad, border), cr.dt)
    try:
        if border:
            pts, ctr, length = U.FAR_BORDER
            eng.set_borders([pts], ctr[None, :], np.array([length]))
        eng.upload_state(cr.loc, cr.vel, cr.waypoint, cr.target_speed, cr.radius, None)
        eng.set_waypoint_stream(U.SEED, U.WORLD_SIDE, cr.thr)
        assert eng.planar == (not cr.z3)
    except Exception:
        eng.close()
        raise
    return eng


def _snapshot(eng):
    loc, vel, wp = eng.state()
    return loc, vel, wp, eng.draw_counts().astype(np.int64)


def _same(a, b, what):
    for name, x, y in zip(("x", "v", "waypoint", "draws"), a, b):
        assert np.array_equal(x, y, equal_nan=True), (what, name, np.flatnonzero((np.asarray(x) != np.asarray(y)).reshape(len(x), -1).any(axis=1))[:6])


def _cell(label, cr, step, check_path, integrate, redraw, ieee, peds, **kw):
    """One crowd through one path under each pedestrian-force setting: the same numbers, then the verdict."""
    snaps = []
    for ped in peds:
        eng = _engine(cr, ped, **kw)
        try:
            step(eng)
            check_path(eng)
            snaps.append(_snapshot(eng))
        finally:
            eng.close()
    for s in snaps[1:]:
        _same(snaps[0], s, f"{label}: pedestrian force {peds[0]} against {peds[1]}")
    return _verdict(label, cr, snaps[0], integrate, redraw, ieee)


def _report(label, results):
    print(f"\n{label}: worst |dv'| / |v'| {max(r[0] for r in results):.2e} (bound 1e-5), worst v' row ulp {max(r[1] for r in results):.2f}")


def _tick_cells(label, n, z3, check_path, peds, shuffle=False, rad=False, launches=None):
    """Host-in-the-loop ticks: the four combinations of integrate / redraw on every (parameter set, threshold)."""
    out = []

    def path(eng):
        check_path(eng)
        if launches is not None:
            assert eng.timing()[2] == launches, (label, eng.timing())
    for pset, thr in SETS:
        cr = U.crowd(n, pset, thr, z3, shuffle)
        for integrate, redraw in FLAGS:
            out.append(_cell(f"{label} {pset} thr={thr} integrate={integrate} redraw={redraw}", cr,
                             lambda eng: eng.tick(integrate=integrate, redraw=redraw), path, integrate, redraw, True, peds, rad=rad))
    _report(label, out)


# ---- sfm_tick_kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
@pytest.mark.parametrize("ipw,team", [(1, 1), (8, 4)])
@pytest.mark.parametrize("n", [65, 257])
def test_ordered_tick_kernel(n, ipw, team, z3, monkeypatch):
    _env(monkeypatch, SFM_SYM=0, SFM_IPW=ipw, SFM_TEAM=team, SFM_CUTOFF=0)
    want = f"sfm_tick_kernel<{ipw},{'true' if z3 else 'false'},false,{team}>"

    def path(eng):
        assert eng.kernel_variant() == want, (eng.kernel_variant(), want)
    _tick_cells(f"ordered N={n} ipw={ipw} team={team} 3d={z3}", n, z3, path, ("off", "stock"), launches=1)


# ---- sfm_pair_sym_kernel + sfm_sym_epilogue_kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["planar", "radius", "3d", "reorder"])
def test_symmetric_pair_kernel_and_epilogue(form, monkeypatch):
    """N = 320.  ``reorder``: SFM_REORDER=1 on a crowd whose rows are dealt over the sites at random -- the stream key is the caller's
    index, and every download comes back in the caller's order (the verdict compares row by row)."""
    reorder = form == "reorder"
    _env(monkeypatch, SFM_SYM=1, SFM_CUTOFF=0, SFM_FUSED=0, SFM_REORDER=1 if reorder else 0)

    def path(eng):
        assert eng.kernel_variant() == SYM, eng.kernel_variant()
    _tick_cells(f"symmetric {form}", 320, form == "3d", path, ("A0", "stock"), shuffle=reorder, rad=form == "radius",
                launches=None if reorder else 2)


# ---- the general fused tick -------------------------------------------------------------------------------------------------------------
FUSED = {"planar": (128, False, {}), "radius": (128, False, {"rad": True}), "3d": (256, True, {}), "geo": (128, False, {"border": True}),
         "N1024-general": (1024, False, {})}


@pytest.mark.parametrize("form", list(FUSED))
def test_fused_tick_general(form, monkeypatch):
    """run(1) straight after upload on the general form (the v_rsq_f32 forms of acceleration_force / capped_velocity), with and without
    redraw.  ``geo``: one border 10 km away, so the launch carries geometry workgroups; ``N1024-general``: SFM_FUSED_LEAN=0."""
    n, z3, kw = FUSED[form]
    _env(monkeypatch, SFM_FUSED=1, SFM_CUTOFF=0, SFM_FUSED_LEAN=0 if n == 1024 else None)
    variant = "sfm_fused_tick_kernel(geo)" if form == "geo" else "sfm_fused_tick_kernel"

    def path(eng):
        assert eng.kernel_variant() == variant and eng.fused_form() == GENERAL, (eng.kernel_variant(), eng.fused_form())
        assert eng.timing()[2] == 2, eng.timing()                 # a launch in front and the tick's own
    out = []
    for pset, thr in SETS:
        cr = U.crowd(n, pset, thr, z3)
        for redraw in (True, False):
            out.append(_cell(f"fused {form} {pset} thr={thr} redraw={redraw}", cr, lambda eng: eng.run(1, redraw=redraw), path, True, redraw,
                             False, ("A0", "stock"), **kw))
    _report(f"fused general {form} (RSQ)", out)


def _resync(label, cr, prev, snap, cfg):
    """One later tick from the device's own previous state, with the exemptions the other multi-tick tests use."""
    loc, vel, wp, draws = prev
    loc, vel = _flat(cr, loc, vel)
    wp3 = np.concatenate([wp, np.zeros((cr.n, 1))], axis=1)
    prm = O.OracleParams.from_config(cfg)
    with np.errstate(all="ignore"):
        oloc, ovel, owp, odraws = O.free_step(loc, vel, wp3, cr.target_speed, cr.radius, np.zeros(cr.n, bool), draws, O.Geometry(), prm, cr.dt,
                                              cr.thr, U.SEED, U.WORLD_SIDE)
    dloc, dvel = _flat(cr, snap[0], snap[1])
    P.check_velocity(dvel, ovel, np.zeros(cr.n), cr.dt)
    assert np.max(np.abs(dloc - oloc)) <= 1e-6 * max(1.0, np.max(np.abs(oloc))) + 1e-6, label
    sure = np.abs(np.linalg.norm(wp - loc[:, :2], axis=1) - cr.thr) > 1e-4
    assert np.allclose(snap[2][sure], owp[sure, :2], rtol=0, atol=1e-4) and np.array_equal(snap[3][sure], odraws[sure]), label


@pytest.mark.parametrize("pset", list(U.PSETS))
def test_fused_tick_three_ticks_cut_as_one_plus_two(pset, monkeypatch):
    """The ties at tick 1 of run(3): cut as 1 + 2 (the verdict after the first call), against run(3) in one call and against 1 + 1 + 1,
    all three bit for bit; ticks 2 and 3 re-synchronised from the device's own state."""
    _env(monkeypatch, SFM_FUSED=1, SFM_CUTOFF=0)
    cr = U.crowd(128, pset, 2.0, False)
    cfg = U.config(pset, "stock")
    engs = [_engine(cr, "stock") for _ in range(3)]
    try:
        cut, whole, single = engs
        cut.run(1, redraw=True)
        assert cut.fused_form() == GENERAL
        first = _snapshot(cut)
        res = _verdict(f"1 + 2 {pset}", cr, first, True, True, False)
        cut.run(2, redraw=True)
        whole.run(3, redraw=True)
        _same(_snapshot(cut), _snapshot(whole), "1 + 2 against 3")
        prev = None
        for t in range(3):
            single.run(1, redraw=True)
            assert single.fused_form() == GENERAL
            snap = _snapshot(single)
            if t == 0:
                _same(snap, first, "tick 1")
            else:
                _resync(f"{pset} tick {t + 1}", cr, prev, snap, cfg)
            prev = snap
        _same(_snapshot(cut), prev, "1 + 2 against 1 + 1 + 1")
    finally:
        for e in engs:
            e.close()
    _report(f"fused 1 + 2 {pset}", [res])


# ---- the lean fused tick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset,thr", SETS)
def test_fused_tick_lean(pset, thr, monkeypatch):
    """N = 1024, a whole planar crowd: the lean form, under the verdict and bit for bit against the general form on the same crowd."""
    cr = U.crowd(1024, pset, thr, False)
    out = []
    for redraw in (True, False):
        snaps = {}
        for lean in (True, False):
            _env(monkeypatch, SFM_FUSED=1, SFM_CUTOFF=0, SFM_FUSED_LEAN=None if lean else 0)
            for ped in ("A0", "stock"):
                eng = _engine(cr, ped)
                try:
                    eng.run(1, redraw=redraw)
                    assert eng.kernel_variant() == "sfm_fused_tick_kernel" and eng.fused_form() == (LEAN if lean else GENERAL), eng.fused_form()
                    snaps[lean, ped] = _snapshot(eng)
                finally:
                    eng.close()
        for key, s in snaps.items():
            _same(snaps[True, "A0"], s, f"lean A0 against {'lean' if key[0] else 'general'} {key[1]}")
        out.append(_verdict(f"lean {pset} thr={thr} redraw={redraw}", cr, snaps[True, "stock"], True, redraw, False))
    _report(f"fused lean {pset} thr={thr} (RSQ)", out)


# ---- step_packed --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
@pytest.mark.parametrize("n", [65, 320])
def test_step_packed(n, z3, monkeypatch):
    """The four combinations of integrate / redraw through sfm_step_packed (N = 65: the ordered kernel, N = 320: the symmetric pair),
    then ``arrived`` on the packed handle after a tick that moved nothing."""
    _env(monkeypatch, SFM_CUTOFF=0, SFM_REORDER=0)
    out = []
    for pset, thr in SETS:
        cr = U.crowd(n, pset, thr, z3)
        rows = np.zeros((n, 9), np.float32)
        rows[:, 0:2], rows[:, 2:4], rows[:, 4:6] = cr.loc[:, :2], cr.vel[:, :2], cr.waypoint[:, :2]
        rows[:, 6], rows[:, 7] = cr.target_speed, cr.radius
        zvz = np.ascontiguousarray(np.stack([cr.loc[:, 2], cr.vel[:, 2]], axis=1), dtype=np.float32) if z3 else None
        for integrate, redraw in FLAGS:
            snaps = []
            for ped in ("A0", "stock"):
                v = np.full((n, 3), np.nan, np.float32)
                eng = SfmEngine(U.config(pset, ped), cr.dt)
                try:
                    eng.set_waypoint_stream(U.SEED, U.WORLD_SIDE, thr)
                    eng.step_packed(rows, zvz, v, integrate=integrate, redraw=redraw)
                    assert eng.kernel_variant().startswith("sfm_tick_kernel<") if n < 256 else eng.kernel_variant() == SYM, eng.kernel_variant()
                    snap = _snapshot(eng)
                    assert np.array_equal(_flat(cr, snap[0], snap[1])[1], _flat(cr, snap[0], v)[1]), "v_out is not the state's v'"
                    snaps.append(snap)
                    if not integrate and not redraw:
                        for t in U.THRESHOLDS:
                            assert np.array_equal(eng.arrived(t), O.arrived(cr.loc, cr.waypoint, t)), f"arrived({t}) on the packed handle"
                finally:
                    eng.close()
            _same(snaps[0], snaps[1], "pedestrian force A0 against stock")
            out.append(_verdict(f"step_packed N={n} 3d={z3} {pset} thr={thr} integrate={integrate} redraw={redraw}", cr, snaps[0], integrate,
                                redraw, True))
    _report(f"step_packed N={n} 3d={z3}", out)


# ---- SfmEngine.arrived ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
def test_arrived_at_every_tie(z3, reorder, monkeypatch):
    """The stand-alone sfm_arrived kernel on an uploaded handle (rows in the caller's order and re-sorted): every tie row, no mask."""
    _env(monkeypatch, SFM_REORDER=reorder)
    rows = 0
    for pset, thr in SETS:
        for n in (65, 320):
            cr = U.crowd(n, pset, thr, z3, bool(reorder))
            eng = _engine(cr, "stock")
            try:
                assert np.array_equal(eng.arrived(thr), cr.arrived), f"arrived({thr})"
                for t in U.THRESHOLDS:
                    got, want = eng.arrived(t), O.arrived(cr.loc, cr.waypoint, t)
                    assert np.array_equal(got, want), [cr.cases[r].name for r in np.flatnonzero(got != want)]
                eng.tick(integrate=False, redraw=False)           # ... and still, once a tick has packed (and maybe re-sorted) the rows
                assert np.array_equal(eng.arrived(thr), cr.arrived), f"arrived({thr}) after a tick"
            finally:
                eng.close()
            rows += n
    print(f"\narrived 3d={z3} reorder={reorder}: {rows} rows, every one on or next to its threshold or its waypoint, no mask")


# ---- the stream's own square: counters beyond 1 ---------------------------------------------------------------------------------------------
STREAM_PATHS = {"ordered": (dict(SFM_SYM=0, SFM_FUSED=0, SFM_CUTOFF=0), 65, "off", lambda e: e.kernel_variant().startswith("sfm_tick_kernel<")),
                "symmetric": (dict(SFM_SYM=1, SFM_FUSED=0, SFM_CUTOFF=0), 320, "stock", lambda e: e.kernel_variant() == SYM),
                "fused-general": (dict(SFM_FUSED=1, SFM_CUTOFF=0), 128, "stock", lambda e: e.fused_form() == GENERAL),
                "fused-lean": (dict(SFM_FUSED=1, SFM_CUTOFF=0), 1024, "stock", lambda e: e.fused_form() == LEAN)}
CALLS = (1, 1, 4, 1, 1)                    # counters 1, 2, 6, 7, 8: d0 = 0, 1 and 7 each met by a call of one tick


def _stream_check(label, cr, wp, draws, ticks):
    """Row 0 (site 0: the origin, inside the stream's square [0, 1)^2) has arrived in every tick; every row's waypoint is the draw its
    counter names, bitwise, or the uploaded one at counter 0."""
    assert draws[0] == ticks, f"{label}: row 0 has counter {draws[0]} after {ticks} ticks"
    hit = np.flatnonzero(draws > 0)
    want = cr.waypoint[:, :2].copy()
    want[hit] = O.redraw_waypoint(hit, draws[hit], U.SEED, U.WORLD_SIDE).astype(np.float64)
    assert np.array_equal(np.asarray(wp, dtype=np.float64), want), f"{label}: after {ticks} ticks"


@pytest.mark.parametrize("pset", list(U.PSETS))
@pytest.mark.parametrize("path", list(STREAM_PATHS))
def test_counters_beyond_one_inside_the_streams_square(path, pset, monkeypatch):
    """The draw counter goes d0 -> d0 + 1 for d0 = 0, 1, 7 (reached by earlier ticks: an upload zeroes the counters) and the new waypoint
    is draw d0 + 1 of the caller's index; after run(4) on top of two ticks the counter is 6."""
    env, n, ped, ok = STREAM_PATHS[path]
    _env(monkeypatch, **env)
    cr = U.crowd(n, pset, 2.0, False, False, U.start_of("on-waypoint-slow", pset))
    assert cr.cases[0].name == "on-waypoint-slow" and not cr.loc[0].any()
    eng = _engine(cr, ped)
    try:
        ticks = 0
        for k in CALLS:
            eng.run(k, redraw=True)
            assert ok(eng), (eng.kernel_variant(), eng.fused_form())
            ticks += k
            _, _, wp, draws = _snapshot(eng)
            _stream_check(f"{path} {pset}", cr, wp, draws, ticks)
    finally:
        eng.close()


# ---- the batch kernel -------------------------------------------------------------------------------------------------------------------
def _batch(crowds, ped):
    return SfmBatch([U.config(c.pset, ped) for c in crowds], [c.dt for c in crowds])


@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
def test_batch_with_waypoint_streams(z3):
    """Scenes of 1, 2, 63, 65 and 300 rows, once per (parameter set, threshold), neighbours on different sets, per-scene seeds and
    thresholds: the four combinations of integrate / redraw, then four more ticks for the counters of each scene's row 0."""
    crowds = U.batch_crowds(z3)
    seeds = [U.SEED + 7 * k for k in range(len(crowds))]
    expect = [U.expectation(c, seed=s) for c, s in zip(crowds, seeds)]
    out = []
    for integrate, redraw in FLAGS:
        got = {}
        for ped in ("off", "stock"):
            b = _batch(crowds, ped)
            try:
                b.upload([c.scene() for c in crowds])
                b.set_waypoint_streams(seeds, U.WORLD_SIDE, [c.thr for c in crowds])
                assert b.planar == (not z3)
                b.tick(integrate=integrate, redraw=redraw)
                got[ped] = [(loc, vel, wp.astype(np.float64), d.astype(np.int64)) for (loc, vel), (wp, d) in zip(b.state(), b.waypoints())]
            finally:
                b.close()
        for k, (c, e) in enumerate(zip(crowds, expect)):
            _same(got["off"][k], got["stock"][k], f"scene {k}: pedestrian force off against stock")
            out.append(_verdict(f"batch scene {k} (N={c.n} {c.pset} thr={c.thr}) integrate={integrate} redraw={redraw}", c, got["off"][k],
                                integrate, redraw, True, e))
    _report(f"batch streams 3d={z3}", out)


def test_batch_counters_beyond_one():
    """Every scene whose row 0 is the slow row on the origin: counters 1, 2, 6, 7, 8 as on the handle, keyed by the scene-local index."""
    crowds = [U.crowd(n, pset, 2.0, False, False, U.start_of("on-waypoint-slow", pset)) for n in U.BATCH_SIZES for pset in U.PSETS]
    b = _batch(crowds, "stock")
    try:
        b.upload([c.scene() for c in crowds])
        b.set_waypoint_streams(U.SEED, U.WORLD_SIDE, 2.0)
        ticks = 0
        for k in CALLS:
            b.run(k, redraw=True)
            ticks += k
            for q, (c, (wp, d)) in enumerate(zip(crowds, b.waypoints())):
                _stream_check(f"batch scene {q}", c, wp, d.astype(np.int64), ticks)
    finally:
        b.close()


@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
def test_batch_with_the_mode_machine(z3):
    """The MODES form's own arrival site: every row walks (mode 1) with its case's target speed; two rows in three hold one queued
    waypoint.  Arrival (strict <, per-scene threshold) pops the queue -- cursor 0 -> 1, the queued waypoint bitwise -- and does nothing
    else on a row that has not arrived; with despawn on, an arrived row with an empty queue is parked (mode 255, v' = 0), and a parked row
    does not arrive again: a second tick leaves its cursor, waypoint and mode alone."""
    crowds = U.batch_crowds(z3)
    despawn = [k % 2 for k in range(len(crowds))]
    plans, queued = [], []
    for c in crowds:
        has = np.arange(c.n) % 3 != 2
        nxt = np.float32(c.loc[:, :2] + np.array([96.0, -48.0])).astype(np.float64)
        plans.append({"mode": np.full(c.n, O.MODE_WALKING_SIDEWALK), "target_speed": c.target_speed, "initial_speed": c.target_speed,
                      "crossing_speed": c.target_speed, "safety_margin": np.zeros(c.n), "next_mode_time": np.zeros(c.n),
                      "queues": [[(nxt[r], False)] if has[r] else [] for r in range(c.n)]})
        queued.append((has, nxt))
    out, parked_rows, popped_rows = [], 0, 0
    got = {}
    for ped in ("off", "stock"):
        b = _batch(crowds, ped)
        try:
            b.upload([c.scene() for c in crowds])
            b.set_modes(plans, despawn_on_arrival=despawn, arrive_thresholds=[c.thr for c in crowds])
            b.run(1)
            first = list(zip(b.state(), b.waypoints(), b.modes()))
            b.run(1)
            got[ped] = (first, list(zip(b.state(), b.waypoints(), b.modes())))
        finally:
            b.close()
    for k, c in enumerate(crowds):
        (loc, vel), (wp, _), (mode, _, cursor) = got["off"][0][k]
        (loc_s, vel_s), (wp_s, _), (mode_s, _, cursor_s) = got["stock"][0][k]
        assert np.array_equal(loc, loc_s) and np.array_equal(vel, vel_s) and np.array_equal(wp, wp_s) and np.array_equal(cursor, cursor_s)
        has, nxt = queued[k]
        hit = c.arrived
        pop = hit & has
        park = hit & ~has & bool(despawn[k])
        assert np.array_equal(cursor, pop.astype(np.int32)), f"scene {k}: cursors"
        assert np.array_equal(mode == 255, park), f"scene {k}: parked rows"
        e = U.expectation(c)
        e.waypoint = np.where(pop[:, None], nxt, c.waypoint[:, :2])
        assert not vel[park].any()
        out.append(_verdict(f"modes scene {k} (N={c.n} {c.pset} thr={c.thr})", c, (loc, vel, wp.astype(np.float64), None), True, True, True, e,
                            skip=park))
        (_, vel2), (wp2, _), (mode2, _, cursor2) = got["off"][1][k]
        assert np.array_equal(mode2[park], mode[park]) and np.array_equal(cursor2[park], cursor[park]) and not vel2[park].any()
        assert np.array_equal(wp2[park], wp[park]), f"scene {k}: a parked row's waypoint moved"
        parked_rows, popped_rows = parked_rows + int(park.sum()), popped_rows + int(pop.sum())
    assert parked_rows >= 20 and popped_rows >= 100
    _report(f"batch modes 3d={z3} ({popped_rows} popped, {parked_rows} parked)", out)
