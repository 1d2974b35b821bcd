"""The speed bound of the tile-pair cutoff on SHARDED ranks (tests/_speed_bound_cases.py: crowds, shard specs, roles; DESIGN.md
sections 3.5 and 4).

On a shard the largest speed of a tile is formed and read where no whole crowd goes: sfm_tick_begin forms the boxes and speeds of
the OWN tiles only and lists the own-own pairs from them, sfm_tick_end forms all tiles again and lists the rest; a pair with another
rank's tile is listed and evaluated one-sided by BOTH ranks, each from its own copy of the other's rows -- {z, vz} included -- which
arrived by the exchange, so the boxes are formed anew every tick; a rank whose bounds are not whole tiles takes the ordered kernel,
whose keep mask then works on tiles it owns part of.  In these crowds a dropped tile pair is the whole pedestrian force of a designed
row, on the rank that dropped it alone.

Each cell is one ``_shards.ShardReplay`` -- G handles in one process, the exchange a device copy -- and one oracle call:
``_parity.check_force`` (``check_velocity`` where the tick integrates) unchanged on every row of the merged crowd, the kernel each
rank ran asserted, and on the symmetric path that every rank's list did cut and did list.  tests/test_speed_bound_shards_host.py
shows on the CPU that the oracle alone makes both ends of every designed pair decide, whatever rank owns them.
Run with  python -m pytest tests/test_speed_bound_shards_gpu.py -m gpu -s."""
import numpy as np
import pytest

import _encounters as E
import _param_sets as psets
import _parity as P
import _shards as SH
import _speed_bound_cases as S

pytestmark = pytest.mark.gpu

KNOBS = ("SFM_SYM", "SFM_IPW", "SFM_TEAM", "SFM_CUTOFF", "SFM_REORDER", "SFM_FUSED", "SFM_PAIR_GEO", "SFM_GEO_SLICES", "SFM_NO_STRAIGHT",
         "SFM_STRIPS", "SFM_RESORT_EVERY")
SYM = "sfm_pair_sym_kernel+sfm_sym_epilogue_kernel"
SPLIT = "sfm_pair_sym_kernel(own|remote)+sfm_sym_epilogue_kernel"


def _env(monkeypatch, cell):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in cell.env:
        monkeypatch.setenv(k, str(v))


def _cfg(rad, forces=S.PED_ONLY):
    return psets.config("stock", forces, use_ped_radius=rad)


def _replay(cell, crowd, cfg, dt, split=False, **kw):
    spec = cell.spec
    return SH.ShardReplay(cfg, crowd.sc, spec.world, layout=spec.partition or None, split=split, resort_every=0, whole=False,
                          bounds=spec.bounds, partition=bool(spec.partition), dt=dt, redraw=False, **kw)


def _check(label, crowd, ref, got):
    """check_force on every row, then what the designed rows -- both ends -- made of it."""
    got = np.asarray(got, dtype=np.float64)
    worst = [float(np.max(np.linalg.norm(got[i] - ref.F[i], axis=1) / ref.term[i])) for i in (crowd.slow, crowd.fast)]
    print(f"\n{label}: worst err/|F| on a designed row: partners {worst[0]:.2e}, fast rows {worst[1]:.2e}")
    P.check_force(label, got, ref.F, ref.absum, ref.expo)


def _listed(rep, spec):
    """on the symmetric path every rank's list did cut and did list: 0 < items < own tiles x n_t"""
    n_t = (rep.n + S.WAVE - 1) // S.WAVE
    for r, e in enumerate(rep.ranks):
        own = (spec.bounds[r + 1] + S.WAVE - 1) // S.WAVE - spec.bounds[r] // S.WAVE
        items = e.engine.pair_work()[0]
        assert 0 < items < own * n_t, (r, items, own, n_t)


def _packing(rep, cell, crowd):
    """'stacks': every rank holds the rows in the order the host file restated (and found to leave the designed tiles)"""
    sc, spec = crowd.sc, cell.spec
    if spec.partition:
        want = SH.pack_order(sc.loc[:, 0], sc.loc[:, 1], rep.n_pad, spec.partition, list(spec.bounds), aspect=rep.aspect, reorder=True)
    else:
        want = S.packing(sc.loc)[0]
    for r, e in enumerate(rep.ranks):
        got = SH.rows_order(SH.packed_rows(e, rep.n)[:, :2], sc.loc[:, :2])
        assert np.array_equal(got, want), f"rank {r}: {int((got != want).sum())} rows are not where the packing puts them"


def _cells(kind):
    out = [c for c in S.SHARD_CELLS if c.kind == kind]
    return out, [c.id for c in out]


PLAIN, PLAIN_IDS = _cells("plain")


@pytest.mark.parametrize("cell", PLAIN, ids=PLAIN_IDS)
def test_recorded_tick_on_every_rank(cell, monkeypatch):
    """Whole tiles per rank: the symmetric path with the own / remote filter on the flat list ('units': 4 | 4 tiles, two each, one
    each) and on the two-level list ('stacks' under the packing: a strip per rank, half a strip each, rank blocks), every rank's
    pedestrian force for its own rows, merged."""
    _env(monkeypatch, cell)
    crowd = S.crowd(cell.spec.crowd)
    cfg = _cfg(cell.rad)
    ref = E.reference(crowd, cfg, 0.05)
    rep = _replay(cell, crowd, cfg, 0.05)
    try:
        if crowd.spec.packed:
            _packing(rep, cell, crowd)
        got = rep.recorded_tick()
        assert rep.variants() == [SYM] * cell.spec.world, rep.variants()
        assert all(e.engine.planar == (not crowd.spec.z3) for e in rep.ranks)
        _listed(rep, cell.spec)
    finally:
        rep.close()
    _check(cell.id, crowd, ref, got)


RAGGED, RAGGED_IDS = _cells("ragged")


@pytest.mark.parametrize("cell", RAGGED, ids=RAGGED_IDS)
def test_ragged_bounds_take_the_ordered_kernel(cell, monkeypatch):
    """Bounds that are not whole tiles (a cut at row 200; cuts at rows 100 and 300, where a wave of eight rows lies in two tiles):
    SFM_SYM=1 and still sfm_tick_kernel on every rank, its keep mask over tiles the rank owns part of -- a fast tile among them, its
    fast row on either side of the cut."""
    _env(monkeypatch, cell)
    crowd = S.crowd(cell.spec.crowd)
    env = dict(cell.env)
    cfg = _cfg(cell.rad)
    ref = E.reference(crowd, cfg, 0.05)
    want = f"sfm_tick_kernel<{env['SFM_IPW']},{'true' if crowd.spec.z3 else 'false'},{'true' if cell.rad else 'false'},{env['SFM_TEAM']}>"
    rep = _replay(cell, crowd, cfg, 0.05)
    try:
        got = rep.recorded_tick()
        assert rep.variants() == [want] * cell.spec.world, rep.variants()
    finally:
        rep.close()
    _check(cell.id, crowd, ref, got)


SPLIT_CELLS, SPLIT_IDS = _cells("split")


@pytest.mark.parametrize("cell", SPLIT_CELLS, ids=SPLIT_IDS)
def test_split_tick_pinned_to_the_oracle_and_to_the_plain_tick(cell, monkeypatch):
    """begin (own tiles' boxes, the own-own list) / exchange / end (all boxes again, the remote list): v' of the merged crowd held to
    the oracle, and bit for bit that of a second replay that takes run(1)."""
    _env(monkeypatch, cell)
    crowd = S.crowd(cell.spec.crowd)
    cfg = _cfg(cell.rad)
    dt = S.DT_SPLIT
    ref = E.reference(crowd, cfg, dt)
    vel, variants = [], []
    for split in (True, False):
        rep = _replay(cell, crowd, cfg, dt, split=split)
        try:
            rep.tick()
            vel.append(rep.merged()[1])
            variants.append(rep.variants())
        finally:
            rep.close()
    assert variants == [[SPLIT] * cell.spec.world, [SYM] * cell.spec.world], variants
    worst = P.check_velocity(vel[0], ref.v_new, ref.expo, dt)
    assert np.array_equal(vel[0], vel[1]), f"{int((vel[0] != vel[1]).any(axis=1).sum())} rows differ from the plain tick's"
    print(f"\n{cell.id}: worst |dv'|/|v'| {worst:.2e}")


def _starters(cell, crowd, **kw):
    """Tick 1 integrates on every rank, the exchange follows, tick 2 records: (merged state after tick 1, merged force of tick 2)."""
    cfg = _cfg(cell.rad, S.CARRY_FORCES)
    rep = _replay(cell, crowd, cfg, S.carry_dt(crowd.spec), split=cell.split, **kw)
    try:
        rep.tick()
        assert rep.variants() == [SPLIT if cell.split else SYM] * cell.spec.world, rep.variants()
        loc, vel, _, _ = rep.merged()
        got = rep.recorded_tick()
        assert rep.variants() == [SYM] * cell.spec.world, rep.variants()
        _listed(rep, cell.spec)
    finally:
        rep.close()
    return loc, vel, got


STARTERS, STARTERS_IDS = _cells("starters")


@pytest.mark.parametrize("cell", STARTERS, ids=STARTERS_IDS)
def test_starters_across_ranks(cell, monkeypatch):
    """The fast rows stand at rest; tick 1 (acceleration and pedestrian force, dt 0.4) brings them to 4.8 m/s on their OWNERS, the
    exchange carries them over, and tick 2 is checked against the oracle on the merged downloaded state: a rank that still holds
    tick 1's speed for a remote tile -- or tick 1's boxes for any -- drops the pair.  The 3-D crowd keeps its v_z."""
    _env(monkeypatch, cell)
    crowd = S.crowd(cell.spec.crowd)
    loc, vel, got = _starters(cell, crowd)
    sp = np.linalg.norm(vel[crowd.fast], axis=1)
    assert (sp > 4.0).all(), sp
    if crowd.spec.starters:
        assert (np.linalg.norm(crowd.sc.vel[crowd.fast], axis=1) == 0.0).all()
    after = S.moved(crowd, loc, vel)
    ref = E._reference(after, _cfg(cell.rad), S.carry_dt(crowd.spec), None)      # (the pedestrian force does not depend on the other forces enabled)
    _check(cell.id, after, ref, got)


def test_a_stale_remote_row_cannot_pass(monkeypatch):
    """Sensitivity control: the 3-D starters replay with {z, vz} left out of the test's own exchange -- every rank then holds the
    other ranks' z and v_z of before tick 1 -- must FAIL the same check."""
    cell = next(c for c in STARTERS if c.spec.crowd == "carry3" and c.spec.world == 2 and not c.split)
    _env(monkeypatch, cell)
    crowd = S.crowd(cell.spec.crowd)
    loc, vel, got = _starters(cell, crowd, exchange_buffers=(0,))
    after = S.moved(crowd, loc, vel)
    ref = E._reference(after, _cfg(cell.rad), S.carry_dt(crowd.spec), None)
    with pytest.raises(AssertionError):
        P.check_force(cell.id, got, ref.F, ref.absum, ref.expo)
