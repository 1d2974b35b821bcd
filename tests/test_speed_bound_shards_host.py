"""The oracle alone must make tests/test_speed_bound_shards_gpu.py meaningful (CPU only, no call into the library;
tests/_speed_bound_cases.py says what the crowds, the shard specs and the roles are).

On a shard a designed pair whose rows belong to two ranks is decided TWICE, one-sided, by each rank from its own copy of the other's
rows: a wrong decision drops one end's whole pedestrian force and leaves the other end right.  So here BOTH ends of every designed
pair must decide -- the partner's row and the fast row:
  * EXPOSURE 0 (``c_oracle.tick(..., theta_tol=P.THETA_TOL)``; 0 as a float32: see ``_ends``);
  * SIZE OF THE TERM: the other row's float64 term on it is at least TERM_FACTOR (1000) times the row's whole check_force allowance;
  * KEPT BY THE TRUE BOUND: the gap between the two tiles' boxes is MARGIN (1 %) inside the true reach;
  * DROPPED BY A WRONG BOUND: the gap is 1 % outside the reach formed with the fast tile's speed replaced by
      - 0, and by the partner tile's speed (the own tile's, read twice) -- what a rank that owns the partner and holds the fast tile as a
        REMOTE one could take (on the rank that owns the fast tile these two replace the slow partner tile's speed, and no speed of a slow
        tile decides anything: what is at stake there is the own tile's speed, next line);
      - the tile's second-largest speed, in 3-D the planar speed, for the starters the speed before tick 1 -- on every rank;
    and, under strips, the gap between the partner's tile and the fast tile's strip is 1 % outside the reach with the speed of any
    other tile of that strip (where the strip holds one fast tile).
The roles table of every shard spec is what its bounds imply (restated here from the device rows: the caller's for 'units',
``packing`` for 'stacks', ``_shards.pack_order`` for the rank blocks), every role occurs with the fast row at lanes 0, 31, 32 and 63
over the cells of the GPU file, and the integrating split-tick cells move v' by at least 100 allowances of check_velocity.
A pair that fails a condition is a failure of the fixture."""
import functools

import numpy as np
import pytest

import _encounters as E
import _param_sets as psets
import _parity as P
import _shards as SH
import _speed_bound_cases as S
from oracle import sfm_oracle as O


@functools.lru_cache(maxsize=None)
def _cfg(rad, forces=S.PED_ONLY):
    return psets.config("stock", forces, use_ped_radius=rad)


def device_order(spec):
    """device row -> caller index under the shard spec's packing"""
    crowd = S.crowd(spec.crowd)
    sc = crowd.sc
    if not crowd.spec.packed:
        return np.arange(sc.n)
    if spec.partition:
        return SH.pack_order(sc.loc[:, 0], sc.loc[:, 1], sc.n, spec.partition, list(spec.bounds),
                             aspect=SH.crowd_aspect(sc.loc[:, 0], sc.loc[:, 1]), reorder=True)
    return S.packing(sc.loc)[0]


def implied(spec):
    """(roles, cut) as the bounds imply them, from the device rows of the designed rows alone."""
    crowd = S.crowd(spec.crowd)
    n = crowd.spec.n
    n_t = (n + S.WAVE - 1) // S.WAVE
    row = np.empty(n, dtype=np.int64)
    row[device_order(spec)] = np.arange(n)
    b = np.asarray(spec.bounds)
    roles, cut = [], []
    for f, s in zip(crowd.fast, crowd.slow):
        rf, rp = int(row[f]), int(row[s])
        kf, kp = (int(np.searchsorted(b, r, side="right")) - 1 for r in (rf, rp))
        tf, tp = rf // S.WAVE, rp // S.WAVE

        def where(own, remote):
            return ("+" if remote > own else "-") + ("w" if 2 * ((remote - own) % n_t) < n_t else "b")
        roles.append(((kf, "oo"),) if kf == kp else tuple(sorted(((kf, "fo" + where(tf, tp)), (kp, "fr" + where(tp, tf))))))
        through = any(S.WAVE * tf < x < S.WAVE * (tf + 1) for x in spec.bounds[1:-1])
        has_part = b[kp] < S.WAVE * (tf + 1) and b[kp + 1] > S.WAVE * tf
        cut.append(("own" if kf == kp else "other") if through and has_part else "")
    return tuple(roles), tuple(cut)


SPECS = list(S.SHARDS.values())


@pytest.mark.parametrize("spec", SPECS, ids=[s.name for s in SPECS])
def test_the_roles_are_what_the_bounds_imply(spec):
    crowd = S.crowd(spec.crowd)
    n = crowd.spec.n
    assert len(spec.bounds) == spec.world + 1 and spec.bounds[0] == 0 and spec.bounds[-1] == n
    assert all(a < b for a, b in zip(spec.bounds, spec.bounds[1:]))                      # every rank owns rows
    roles, cut = implied(spec)
    assert spec.roles == roles, (spec.name, roles)
    assert (spec.cut or ("",) * crowd.n_pairs) == cut, (spec.name, cut)
    assert all(r in S.ROLES for pair in spec.roles for _, r in pair)
    order = device_order(spec)
    if crowd.spec.packed:
        # the packing -- the plain one and the rank blocks' -- leaves every designed tile as one device tile, at its index
        tile_of = np.empty(n, dtype=np.int64)
        tile_of[order] = np.arange(n) // S.WAVE
        assert np.array_equal(tile_of[crowd.fast], crowd.tiles[:, 0]) and np.array_equal(tile_of[crowd.slow], crowd.tiles[:, 1])
        assert np.array_equal(order, np.arange(n))                                       # (and, unshuffled, every row where the caller has it)
        assert S.packing(crowd.sc.loc)[1] == crowd.spec.shape[1]
        assert spec.aligned
    if spec.partition:
        assert spec.partition[0] * spec.partition[1] == spec.world
    if spec.world == 8 and n % S.WAVE == 0:
        assert all(len(pair) == 2 for pair in spec.roles)                                # one tile each: no own-own pair exists
    if crowd.spec.packed and spec.world == 2:
        assert all(len(pair) == 2 for pair in spec.roles)                                # one strip per rank: every pair is remote on both sides


def test_the_cells_cover_every_role_at_every_lane():
    """... and the worlds, bounds, dimensions, radii, knobs and tick forms the GPU file is there for.  Editing a shard spec or a cell
    so that a role, a lane or a direction goes missing fails here."""
    seen = set()
    for cell in S.SHARD_CELLS:
        spec = cell.spec
        crowd = S.crowd(spec.crowd)
        row = np.empty(crowd.spec.n, dtype=np.int64)
        row[device_order(spec)] = np.arange(crowd.spec.n)
        for f, pair in zip(crowd.fast, spec.roles):
            seen |= {(role, int(row[f] % S.WAVE)) for _, role in pair}
    missing = [(r, l) for r in S.ROLES for l in S.ROLE_LANES if (r, l) not in seen]
    assert not missing, missing
    cells = S.SHARD_CELLS
    assert len({c.id for c in cells}) == len(cells) and all(c.shard in S.SHARDS for c in cells)
    z3 = lambda c: S.SPECS[c.spec.crowd].z3                                               # noqa: E731
    units = [c for c in cells if c.kind == "plain" and not S.SPECS[c.spec.crowd].packed]
    for world in (2, 4, 8):
        mine = [c for c in units if c.spec.world == world]
        assert {(z3(c), c.rad) for c in mine} == {(a, b) for a in (False, True) for b in (False, True)}, world
        assert {S.SPECS[c.spec.crowd].n for c in mine} == {512, 529}, world
        assert all(c.spec.aligned for c in mine)
    ragged = [c for c in cells if c.kind == "ragged"]
    assert {(c.spec.world, c.spec.bounds[1:-1]) for c in ragged} == {(2, (200,)), (3, (100, 300))}
    assert {z3(c) for c in ragged} == {False, True} and not any(c.spec.aligned for c in ragged)
    # a cut through a fast tile, its fast row on the side of the rank that owns the partner and on the other rank's: planar and 3-D
    assert {z3(c) for c in ragged if "own" in c.spec.cut} == {False, True} and {z3(c) for c in ragged if "other" in c.spec.cut} == {False, True}
    stacks = [c for c in cells if c.kind == "plain" and S.SPECS[c.spec.crowd].packed and not c.spec.partition]
    assert {(c.spec.world, dict(c.env)["SFM_STRIPS"], z3(c), c.spec.crowd.startswith("strip-w15")) for c in stacks} == \
        {(w, s, z, q) for w in (2, 4) for s in (0, 1) for z in (False, True) for q in (False, True)}
    assert all(S.SPECS[c.spec.crowd].n == 2048 and S.SPECS[c.spec.crowd].shape == (2, 16) for c in stacks)
    assert [(c.spec.partition, c.spec.world, S.SPECS[c.spec.crowd].n) for c in cells if c.spec.partition] == [((2, 2), 4, 2048)]
    split = [c for c in cells if c.kind == "split"]
    assert {(c.spec.world, S.SPECS[c.spec.crowd].packed) for c in split} == {(w, p) for w in (2, 4) for p in (False, True)}
    assert {c.spec.world for c in split if S.SPECS[c.spec.crowd].cap_free} == {2, 4}
    assert all(c.split for c in split)
    starters = [c for c in cells if c.kind == "starters"]
    assert {(c.spec.crowd, c.spec.world, c.split) for c in starters} == \
        {(c, w, s) for c in ("starters", "carry3") for w in (2, 4) for s in (False, True)}
    assert all(dict(c.env)["SFM_SYM"] == 1 and dict(c.env)["SFM_CUTOFF"] == 1 for c in cells)


def _ends(label, crowd, ref, rad):
    """Exposure and size of the term on BOTH ends of every designed pair.  Returns the smallest term / allowance, per end."""
    sc = crowd.sc
    out = []
    for what, i, j in (("partner's row", crowd.slow, crowd.fast), ("fast row", crowd.fast, crowd.slow)):
        t = E.pair_terms(sc.loc[i], sc.vel[i], sc.radius[i], sc.loc[j], sc.vel[j], sc.radius[j], rad)
        allow = P.RTOL * np.maximum(ref.term[i], np.nan_to_num(ref.absum[i])) + P.ATOL
        # 0 -- in the kernel's arithmetic.  At 5 m/s (3-D: a relative v_z of 6 m/s) B is about 4 m, so a row of ANOTHER site that happens
        # to lie where theta changes sign (a window of 2e-5 rad, 3 cm wide at 1500 m: one fast row in three has such a row) has a term of
        # exp(-1500 / 4), 1e-56 ... 1e-170 m/s^2, where a slow pair's underflows to 0 in float64.  Below 1.4e-45 the float32 is 0.
        assert (np.float32(np.nan_to_num(ref.expo[i], nan=1.0)) == 0.0).all(), (label, what, ref.expo[i])
        assert (np.nan_to_num(t["expo"], nan=1.0) == 0.0).all(), (label, what)
        ratio = t["norm"] / allow
        assert (ratio >= S.TERM_FACTOR).all(), (label, what, t["norm"], allow)
        out.append((float(ratio.min()), float(t["norm"].min())))
    return out


def _reaches(label, spec, crowd, rs, rad, old=None, moved=False):
    """Kept by the true bound, dropped by every wrong one, per rank that decides the pair."""
    z3 = crowd.spec.z3
    slow = S.SLOW[z3] * (1.0 + S.MARGIN if moved else 1.0)              # (a tick's forces move a slow row's speed by 1e-6)
    for k, ((tf, tp), ranks) in enumerate(zip(crowd.tiles, spec.roles)):
        gap = S.box_gap(rs.box[tf], rs.box[tp])
        reach = functools.partial(S.reach, rad=rad, r_max=rs.r_max)
        assert gap <= (1 - S.MARGIN) * reach(rs.vmax[tf], rs.vmax[tp]), (label, k, gap)
        assert rs.v2nd[tf] <= slow and rs.vmax[tp] <= slow, (label, k, rs.v2nd[tf], rs.vmax[tp])       # one fast row, a slow partner tile
        for rank, role in ranks:
            wrong = {"second largest": reach(rs.v2nd[tf], rs.vmax[tp])}
            if z3:
                wrong["planar speed"] = reach(rs.vmax_planar[tf], rs.vmax[tp])
            if old is not None:
                wrong["speed before tick 1"] = reach(old.vmax[tf], rs.vmax[tp])
            if role.startswith("fr"):                                   # the fast tile is this rank's REMOTE one
                wrong["remote tile's speed as 0"] = reach(0.0, rs.vmax[tp])
                wrong["own tile's speed twice"] = reach(rs.vmax[tp], rs.vmax[tp])
            for what, r in wrong.items():
                assert gap >= (1 + S.MARGIN) * r, (label, k, rank, role, what, gap, r)
        if rs.tps > 1:
            s = rs.strip_of(tf)
            sgap = S.box_gap(rs.box[tp], rs.strip_box(s))
            assert sgap <= (1 - S.MARGIN) * reach(rs.vmax[tp], max(rs.vmax[u] for u in rs.strip_tiles(s))), (label, k)
            others = [u for u in rs.strip_tiles(s) if u != tf]
            if all(rs.vmax[u] <= slow for u in others):               # the strip's one fast tile: its strip bound is at stake
                for u in others:
                    assert sgap >= (1 + S.MARGIN) * reach(rs.vmax[tp], rs.vmax[u]), (label, k, u)


DECIDING = [c for c in S.SHARD_CELLS if c.kind != "starters"]


@pytest.mark.parametrize("cell", DECIDING, ids=[c.id for c in DECIDING])
def test_both_ends_of_every_designed_pair_decide(cell):
    spec = cell.spec
    crowd = S.crowd(spec.crowd)
    ref = E.reference(crowd, _cfg(cell.rad), 0.05)
    ends = _ends(cell.id, crowd, ref, cell.rad)
    _reaches(cell.id, spec, crowd, S.restate(crowd), cell.rad)
    if crowd.spec.packed:                # a strip with ONE fast tile in every stacks crowd: the strip bound is at stake somewhere
        rs = S.restate(crowd)
        assert any(sum(rs.vmax[u] > S.SLOW[crowd.spec.z3] for u in rs.strip_tiles(rs.strip_of(tf))) == 1 for tf, _ in crowd.tiles)
    print(f"\n{cell.id}: smallest term / allowance: partner's rows {ends[0][0]:.1e} ({ends[0][1]:.2e} m/s^2), fast rows {ends[1][0]:.1e} "
          f"({ends[1][1]:.2e} m/s^2)")


SPLIT = [c for c in S.SHARD_CELLS if c.kind == "split"]


@pytest.mark.parametrize("cell", SPLIT, ids=[c.id for c in SPLIT])
def test_the_designed_term_moves_the_split_ticks_velocity(cell):
    """v' of the oracle with and without the designed term differ by at least VELOCITY_FACTOR (100) allowances of check_velocity at
    the cell's dt on the partner's row (at dt = 0.05 they reach 40-60: DT_CARRY it is); on the fast row's end by that in the crowd
    whose fast rows no cap touches, by VELOCITY_FACTOR_FAST elsewhere (``_speed_bound_cases`` says why)."""
    crowd = S.crowd(cell.spec.crowd)
    sc, dt = crowd.sc, S.DT_SPLIT
    assert dt in (0.05, S.DT_CARRY)
    ref = E.reference(crowd, _cfg(cell.rad), dt)
    for what, i, j in (("partner's row", crowd.slow, crowd.fast), ("fast row", crowd.fast, crowd.slow)):
        t = E.pair_terms(sc.loc[i], sc.vel[i], sc.radius[i], sc.loc[j], sc.vel[j], sc.radius[j], cell.rad)
        without = O.new_velocities(sc.vel[i], ref.F[i] - t["F"], sc.target_speed[i], dt)
        moved = np.linalg.norm(ref.v_new[i] - without, axis=1)
        allow = P.RTOL * np.linalg.norm(ref.v_new[i], axis=1) + 1e-12                          # check_velocity's, exposure 0
        factor = S.VELOCITY_FACTOR if what == "partner's row" or crowd.spec.cap_free else S.VELOCITY_FACTOR_FAST
        assert (moved >= factor * allow).all(), (cell.id, what, moved / allow)
        print(f"\n{cell.id}: {what}: the designed term moves v' by {np.min(moved / allow):.0f}-{np.max(moved / allow):.0f} allowances")


STARTERS = [c for c in S.SHARD_CELLS if c.kind == "starters" and not c.split]


@pytest.mark.parametrize("cell", STARTERS, ids=[c.id for c in STARTERS])
def test_starters_decide_on_both_ends_after_their_first_tick(cell):
    """The oracle's tick (acceleration and pedestrian force) moves the crowd on; on the state after it both ends of every designed
    pair decide, and a rank that still holds the fast tile's speed of before the tick ('starters': 0) drops the pair."""
    spec = cell.spec
    crowd = S.crowd(spec.crowd)
    cfg = _cfg(cell.rad, S.CARRY_FORCES)
    sc, dt = crowd.sc, S.carry_dt(crowd.spec)
    v1 = E.reference(crowd, cfg, dt).v_new
    sp = np.linalg.norm(v1[crowd.fast], axis=1)
    if crowd.spec.starters:
        assert (sp >= 4.0).all() and (np.linalg.norm(sc.vel[crowd.fast], axis=1) == 0.0).all(), sp
    else:
        assert crowd.spec.z3 and (np.abs(v1[crowd.fast, 2]) >= 5.0).all(), v1[crowd.fast]
    after = S.moved(crowd, S._f32(sc.loc + dt * v1), S._f32(v1))
    ref = E._reference(after, _cfg(cell.rad), dt, None)
    ends = _ends(cell.id, after, ref, cell.rad)
    _reaches(cell.id, spec, after, S.restate(after), cell.rad, old=S.restate(crowd) if crowd.spec.starters else None, moved=True)
    print(f"\n{cell.id}: fast rows at {sp.min():.2f}-{sp.max():.2f} m/s after tick 1; smallest term / allowance: partner's rows "
          f"{ends[0][0]:.1e}, fast rows {ends[1][0]:.1e}")
