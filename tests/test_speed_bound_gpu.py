"""The speed bound of the tile-pair cutoff, one fast row per tile (tests/_speed_bound_cases.py; DESIGN.md sections 3.5 and 4).

The cutoff's reach grows with the largest speed of the two tiles, and that speed is formed in four places -- sfm_tile_bounds_kernel,
sfm_tile_strip_bounds_kernel, sfm_strip_bounds_kernel, the epilogue's carry of the next state's bounds -- and read in five: the flat
list, the two-level list, the epilogue's partner enumeration, the pair kernel's per-step reach test, the ordered kernel's keep mask.
In these crowds a fast row heads for a slow partner in ANOTHER tile, across a gap between the reach without the fast row and the
true reach: any of them wrong, and the tile pair -- the partner's whole pedestrian force -- is dropped.

Each cell is one engine, one recorded tick and one oracle call, ``_parity.check_force`` unchanged on every row; it asserts the
kernel it ran and, on the symmetric path, that the list did cut.  tests/test_speed_bound_host.py shows on the CPU that the oracle
alone makes every crowd decide.  Run with  python -m pytest tests/test_speed_bound_gpu.py -m gpu -s."""
import numpy as np
import pytest

import _encounters as E
import _param_sets as psets
import _parity as P
import _speed_bound_cases as S
from carla_social_force_model_amd.engine import SfmEngine

pytestmark = pytest.mark.gpu

KNOBS = ("SFM_SYM", "SFM_IPW", "SFM_TEAM", "SFM_CUTOFF", "SFM_REORDER", "SFM_FUSED", "SFM_PAIR_GEO", "SFM_GEO_SLICES", "SFM_NO_STRAIGHT",
         "SFM_STRIPS", "SFM_RESORT_EVERY")


def _env(monkeypatch, cell):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in cell.env:
        monkeypatch.setenv(k, str(v))


def _cfg(rad, forces=S.PED_ONLY):
    return psets.config("stock", forces, use_ped_radius=rad)


def _check(label, crowd, ref, got):
    """check_force on every row, then what the designed rows made of it."""
    i = crowd.slow
    err = np.linalg.norm(np.asarray(got, dtype=np.float64)[i] - ref.F[i], axis=1)
    print(f"\n{label}: partners' rows: |F| {ref.term[i].min():.2e}-{ref.term[i].max():.2e} m/s^2, worst err/|F| {np.max(err / ref.term[i]):.2e}")
    P.check_force(label, got, ref.F, ref.absum, ref.expo)


def _all_items(n):
    n_t = (n + S.WAVE - 1) // S.WAVE
    return n_t * (n_t - 1) // 2 + (n_t + 1) // 2


def _upload(eng, sc):
    eng.upload_state(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, None)


def _cells(kind):
    out = [c for c in S.CELLS if c.kind == kind]
    return out, [c.id for c in out]


SYM, SYM_IDS = _cells("sym")


@pytest.mark.parametrize("cell", SYM, ids=SYM_IDS)
def test_symmetric_kernel_under_the_list(cell, monkeypatch):
    """Flat list (sfm_tile_bounds_kernel; 'units' crowds, caller's tiles) and two-level list ('stacks' crowds under the packing, two
    strips of sixteen tiles: planar the merged sfm_tile_strip_bounds_kernel, 3-D sfm_tile_bounds_kernel + sfm_strip_bounds_kernel)."""
    _env(monkeypatch, cell)
    crowd = S.crowd(cell.crowd)
    spec = crowd.spec
    cfg = _cfg(cell.rad)
    ref = E.reference(crowd, cfg, 0.05)
    eng = SfmEngine(cfg, 0.05)
    try:
        _upload(eng, crowd.sc)
        assert eng.planar == (not spec.z3)
        eng.tick(record=True)
        assert eng.kernel_variant() == "sfm_pair_sym_kernel+sfm_sym_epilogue_kernel", eng.kernel_variant()
        # bounds [+ strip bounds] + list + pair kernel + epilogue; the merged launch holds tile and strip bounds
        strips = dict(cell.env)["SFM_STRIPS"]
        assert eng.timing()[2] == 4 + (1 if strips and spec.z3 else 0), eng.timing()
        got = eng.forces("pedestrian_force")
        items = eng.pair_work()
    finally:
        eng.close()
    assert 0 < items[0] < _all_items(spec.n), items
    _check(cell.id, crowd, ref, got)


ORD, ORD_IDS = _cells("ordered")


@pytest.mark.parametrize("cell", ORD, ids=ORD_IDS)
def test_ordered_kernel_keep_mask(cell, monkeypatch):
    """sfm_tick_kernel under the cutoff: a wave keeps a bit per partner tile from the two tiles' boxes and largest speeds.  (It builds
    no list, so there is no work count to read; a mask that kept everything could not fail here, one that drops a designed pair does.)"""
    _env(monkeypatch, cell)
    crowd = S.crowd(cell.crowd)
    env = dict(cell.env)
    cfg = _cfg(cell.rad)
    ref = E.reference(crowd, cfg, 0.05)
    want = f"sfm_tick_kernel<{env['SFM_IPW']},{'true' if crowd.spec.z3 else 'false'},{'true' if cell.rad else 'false'},{env['SFM_TEAM']}>"
    eng = SfmEngine(cfg, 0.05)
    try:
        _upload(eng, crowd.sc)
        eng.tick(record=True)
        assert eng.kernel_variant() == want, eng.kernel_variant()
        assert eng.timing()[2] == 2, eng.timing()                 # the bounds and the tick's own launch
        got = eng.forces("pedestrian_force")
    finally:
        eng.close()
    _check(cell.id, crowd, ref, got)


CARRIED, CARRIED_IDS = _cells("carried")


@pytest.mark.parametrize("cell", CARRIED, ids=CARRIED_IDS)
def test_bounds_carried_by_the_epilogue(cell, monkeypatch):
    """The starters stand at rest; one integrating tick (acceleration and pedestrian force, dt 0.4, target speed 6 m/s, the cap at
    7.8 untouched) brings them to 4.8 m/s and its epilogue leaves the next tick's boxes and largest speeds.  The next tick takes them
    -- one launch fewer -- and is checked against the oracle on the downloaded state: a bound carried from the velocity before the
    tick drops every designed pair.  The 3-D crowd (dt 2^-7, the cap above its fast rows): they keep their v_z but for 1.6 %, and a
    carried bound formed without it drops the pairs."""
    _env(monkeypatch, cell)
    crowd = S.crowd(cell.crowd)
    cfg = _cfg(cell.rad, S.CARRY_FORCES)
    dt = S.carry_dt(crowd.spec)
    eng = SfmEngine(cfg, dt)
    try:
        _upload(eng, crowd.sc)
        eng.run(1)
        assert eng.kernel_variant() == "sfm_pair_sym_kernel+sfm_sym_epilogue_kernel", eng.kernel_variant()
        assert eng.timing()[2] == 4, eng.timing()                 # bounds, list, pair kernel, epilogue
        loc, vel, _ = eng.state()
        eng.tick(record=True)
        assert eng.timing()[2] == 3, eng.timing()                 # the carried boxes: no bounds launch
        got = eng.forces("pedestrian_force")
        items = eng.pair_work()
    finally:
        eng.close()
    sp = np.linalg.norm(vel[crowd.fast], axis=1)
    assert (sp > 4.0).all(), sp
    if crowd.spec.starters:
        assert (np.linalg.norm(crowd.sc.vel[crowd.fast], axis=1) == 0.0).all()
    after = S.moved(crowd, loc, vel)
    ref = E._reference(after, _cfg(cell.rad), dt, None)            # (the pedestrian force does not depend on the other forces enabled)
    assert 0 < items[0] < _all_items(crowd.spec.n), items
    _check(cell.id, after, ref, got)


SHIPPED, SHIPPED_IDS = _cells("shipped")


@pytest.mark.parametrize("cell", SHIPPED, ids=SHIPPED_IDS)
def test_as_shipped(cell, monkeypatch):
    """N = 4160 and no knob set: the default packing (which leaves the designed tiles, whatever the caller's order: asserted by the
    host file), the automatic cutoff above 4096, rows in a shuffled caller order, so the downloads' permutation is in play."""
    _env(monkeypatch, cell)
    crowd = S.crowd(cell.crowd)
    cfg = _cfg(cell.rad)
    ref = E.reference(crowd, cfg, 0.05)
    eng = SfmEngine(cfg, 0.05)
    try:
        _upload(eng, crowd.sc)
        eng.tick(record=True)
        assert "sym" in eng.kernel_variant(), eng.kernel_variant()
        got = eng.forces("pedestrian_force")
        items = eng.pair_work()
        loc, _, _ = eng.state()
    finally:
        eng.close()
    assert np.array_equal(loc[:, :2], crowd.sc.loc[:, :2])        # caller order
    assert 0 < items[0] < _all_items(crowd.spec.n), items
    _check(cell.id, crowd, ref, got)
