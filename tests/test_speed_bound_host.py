"""The oracle alone must make tests/test_speed_bound_gpu.py meaningful (CPU only; tests/_speed_bound_cases.py says what the crowds are).

For every designed pair -- a fast row and its partner in a slow tile across the gap -- of every crowd the GPU file runs (both files
read ``_speed_bound_cases.CELLS``), stock parameters, the radius setting of the cell:
  * EXPOSURE: the partner's row has exposure 0 (``c_oracle.tick(..., theta_tol=P.THETA_TOL)``);
  * SIZE OF THE TERM: the fast row's float64 term on it (``_encounters.pair_terms``) is at least 1000 times the row's whole
    check_force allowance RTOL max(|F|, absum) + ATOL;
  * KEPT BY THE TRUE BOUND: the gap between the two tiles' boxes is below the true reach by at least 1 % (and so is the gap between
    the partner's tile and the fast tile's strip, under the strip's true bound);
  * DROPPED BY A WRONG BOUND: the gap is above the reach by at least 1 % with the fast tile's largest speed replaced by its second
    largest, in 3-D with the planar speeds alone, for strips with the bound of ANY other tile of the strip, and in the carried-bounds
    crowd with the bound of the state before the tick.
Boxes, speeds, gaps and reaches come from ``_speed_bound_cases.restate``: float64, from the coordinates, no call into the library.
A pair that fails a condition is a failure of the fixture.  The last tests assert that the lanes, tile positions and roles the
fixture is there for all occur in the cells.
"""
import functools

import numpy as np
import pytest

import _encounters as E
import _param_sets as psets
import _parity as P
import _speed_bound_cases as S


@functools.lru_cache(maxsize=None)
def _cfg(rad, forces=S.PED_ONLY):
    return psets.config("stock", forces, use_ped_radius=rad)


def _bounds(label, crowd, rs, rad, old=None, moved=False):
    """Conditions 3 and 4 for every designed pair of ``crowd`` under the restatement ``rs``; ``old``: the restatement of the state a
    wrongly carried bound would come from; ``moved``: the state is one tick on from the designed one."""
    for k, (tf, ts) in enumerate(crowd.tiles):
        gap = S.box_gap(rs.box[tf], rs.box[ts])
        true = S.reach(rs.vmax[tf], rs.vmax[ts], rad, rs.r_max)
        assert gap <= (1 - S.MARGIN) * true, (label, k, gap, true)
        wrong = {"second largest": S.reach(rs.v2nd[tf], rs.vmax[ts], rad, rs.r_max)}
        if crowd.spec.z3:
            wrong["planar speed"] = S.reach(rs.vmax_planar[tf], rs.vmax[ts], rad, rs.r_max)
        if old is not None:
            wrong["old velocity"] = S.reach(old.vmax[tf], rs.vmax[ts], rad, rs.r_max)
        for what, r in wrong.items():
            assert gap >= (1 + S.MARGIN) * r, (label, k, what, gap, r)
        slow = S.SLOW[crowd.spec.z3] * (1.0 + S.MARGIN if moved else 1.0)      # (a tick's forces move a slow row's speed by 1e-6)
        assert rs.v2nd[tf] <= slow and rs.vmax[ts] <= slow, (label, k)                 # one fast row, a slow partner tile
        if rs.tps > 1:
            s = rs.strip_of(tf)
            sgap = S.box_gap(rs.box[ts], rs.strip_box(s))
            others = [u for u in rs.strip_tiles(s) if u != tf]
            assert sgap <= (1 - S.MARGIN) * S.reach(rs.vmax[ts], max(rs.vmax[u] for u in rs.strip_tiles(s)), rad, rs.r_max), (label, k)
            if rs.strip_of(ts) < s:      # (the list keeps the pair under the partner's tile: the fast tile's strip bound is at stake)
                for u in others:
                    assert sgap >= (1 + S.MARGIN) * S.reach(rs.vmax[ts], rs.vmax[u], rad, rs.r_max), (label, k, u)


def _terms(label, crowd, ref, rad):
    """Conditions 1 and 2 on the partner's row of every designed pair.  Returns the smallest term / allowance."""
    sc = crowd.sc
    i, j = crowd.slow, crowd.fast
    t = E.pair_terms(sc.loc[i], sc.vel[i], sc.radius[i], sc.loc[j], sc.vel[j], sc.radius[j], rad)
    allow = P.RTOL * np.maximum(ref.term[i], np.nan_to_num(ref.absum[i])) + P.ATOL
    assert (np.nan_to_num(ref.expo[i], nan=1.0) == 0.0).all(), (label, ref.expo[i])
    ratio = t["norm"] / allow
    assert (ratio >= S.TERM_FACTOR).all(), (label, t["norm"], allow)
    return float(ratio.min()), float(t["norm"].min())


CELLS = [c for c in S.CELLS if c.kind != "carried"]


@pytest.mark.parametrize("cell", CELLS, ids=[c.id for c in CELLS])
def test_every_designed_pair_decides(cell):
    crowd = S.crowd(cell.crowd)
    rs = S.restate(crowd)
    if crowd.spec.packed:                          # the packing leaves the designed tiles, whatever the caller's order
        rows = np.arange(crowd.spec.n)
        tile_of = np.empty(crowd.spec.n, dtype=np.int64)
        tile_of[rs.order] = rows // S.WAVE
        assert rs.tps == crowd.spec.shape[1]
        assert np.array_equal(tile_of[crowd.fast], crowd.tiles[:, 0]) and np.array_equal(tile_of[crowd.slow], crowd.tiles[:, 1])
        if not crowd.spec.shuffled:
            assert np.array_equal(rs.order, rows)
    ref = E.reference(crowd, _cfg(cell.rad), 0.05)
    worst, term = _terms(cell.id, crowd, ref, cell.rad)
    _bounds(cell.id, crowd, rs, cell.rad)
    print(f"\n{cell.id}: {crowd.n_pairs} designed pairs, smallest term {term:.2e} m/s^2 = {worst:.1e} allowances")


CARRIED = [c for c in S.CELLS if c.kind == "carried"]


@pytest.mark.parametrize("cell", CARRIED, ids=[c.id for c in CARRIED])
def test_carried_bounds_crowd_decides_after_its_first_tick(cell):
    """The oracle's tick (acceleration and pedestrian force) moves the crowd on; on the state after it the four conditions hold.
    'starters': the fast rows stand at rest at tick 0 and the tick (dt = DT_CARRY) brings them to several m/s, under the cap -- a
    bound formed from the velocities before the tick drops the pair.  The 3-D crowd (dt = DT_CARRY_3D, the cap above the fast rows):
    v_z decays by 1.6 % (the acceleration force's z component is -v_z / tau), and a carried bound without v_z drops the pair."""
    crowd = S.crowd(cell.crowd)
    cfg = _cfg(cell.rad, S.CARRY_FORCES)
    sc, dt = crowd.sc, S.carry_dt(crowd.spec)
    first = E.reference(crowd, cfg, dt)
    v1 = first.v_new
    sp = np.linalg.norm(v1[crowd.fast], axis=1)
    if crowd.spec.starters:
        assert (sp >= 4.0).all() and (sp < 0.9 * cfg.get("max_speed_factor", 1.3) * S.STARTER_SPEED).all(), sp       # the cap does not touch them
        assert (np.linalg.norm(sc.vel[crowd.fast], axis=1) == 0.0).all()
    else:
        assert crowd.spec.z3 and (np.abs(v1[crowd.fast, 2]) >= 5.0).all(), v1[crowd.fast]
    after = S.moved(crowd, S._f32(sc.loc + dt * v1), S._f32(v1))
    # (the pedestrian force alone: it is the record the GPU cell checks, and its absum then carries no acceleration term)
    ref = E._reference(after, _cfg(cell.rad), dt, None)
    worst, term = _terms(cell.id, after, ref, cell.rad)
    _bounds(cell.id, after, S.restate(after), cell.rad, old=S.restate(crowd) if crowd.spec.starters else None, moved=True)
    print(f"\n{cell.id}: fast rows at {sp.min():.2f}-{sp.max():.2f} m/s after the tick, smallest term {term:.2e} m/s^2 = {worst:.1e} allowances")


def test_the_cells_cover_lanes_tile_positions_and_roles():
    sym = [S.crowd(c.crowd) for c in S.CELLS if c.kind == "sym"]
    units = [c for c in sym if not c.spec.packed]
    lanes = {int(r % S.WAVE) for c in units for r in c.fast}
    assert {0, 1, 31, 32, 63} <= lanes, sorted(lanes)
    for z3 in (False, True):
        mine = [c for c in units if c.spec.z3 == z3]
        assert any(c.spec.n % S.WAVE == 17 and (c.fast == c.spec.n - 1).any() for c in mine)                 # the ragged tile's last index
        full = [c for c in mine if c.spec.n % S.WAVE == 0]
        n_t = full[0].spec.n // S.WAVE
        fast_tiles = {int(t) for c in full for t in c.tiles[:, 0]}
        assert fast_tiles == set(range(n_t)), sorted(fast_tiles)                                               # every tile is the fast one somewhere
        seen = set()
        for c in full:
            for tf, ts in c.tiles:
                ahead = (ts - tf) % n_t
                seen.add(("above" if ts > tf else "below", "within" if 2 * ahead < n_t else "beyond"))
        assert seen == {(a, b) for a in ("above", "below") for b in ("within", "beyond")}, seen
        assert any({0, n_t - 1} <= set(c.tiles[:, 0].tolist()) and (set(c.tiles[:, 0].tolist()) - {0, n_t - 1}) for c in full)
        # strips: a fast tile in the middle of its strip, and one in the sixteenth wave's share of the merged launch
        strips = [c for c in sym if c.spec.packed and c.spec.z3 == z3]
        pos = set()
        for c in strips:
            tps = c.spec.shape[1]
            pos |= {int(tf % tps) for tf, ts in c.tiles if ts < tf}
            fast_strip1 = [tf for tf, ts in c.tiles if tf >= tps]
            assert len(fast_strip1) == 1, c.spec.name                                                         # ONE fast tile where the strip bound is at stake
        assert 15 in pos and any(0 < q < 15 for q in pos), pos
    for kind, rads in (("sym", {False, True}), ("ordered", {False, True})):
        for z3 in (False, True):
            assert {c.rad for c in S.CELLS if c.kind == kind and S.SPECS[c.crowd].z3 == z3} == rads
    assert len({c.env for c in S.CELLS if c.kind == "ordered"}) == 2
    assert any(c.kind == "shipped" and S.SPECS[c.crowd].shuffled and S.SPECS[c.crowd].n == 4160 and not c.env for c in S.CELLS)
    assert len({c.id for c in S.CELLS}) == len(S.CELLS)
