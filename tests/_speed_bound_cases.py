"""Crowds with ONE FAST ROW PER TILE, for the speed bound of the tile-pair cutoff (tests/test_speed_bound_host.py on the CPU,
tests/test_speed_bound_gpu.py on the GPU; on sharded ranks tests/test_speed_bound_shards_host.py and
tests/test_speed_bound_shards_gpu.py, whose shard specs, roles and cells stand at the end of this file; DESIGN.md sections 3.5 and 4).
No GPU code here, and no call into the library.

The cutoff drops a tile pair whose boxes are farther apart than  gamma 41 ln2 1.001 (1 + lambda (vmax_a + vmax_b)) (+ 2 r_max 1.001),
vmax the largest speed of a tile.  Every other crowd that runs under the cutoff walks at <= 1.6 m/s, evenly over the tiles, with its
partners within 3 m -- inside the reach even at vmax = 0 -- so a wrong vmax changes nothing there.  Here:

  * a tile is 64 consecutive device rows on an 8 x 8 grid of 8 m pitch (a 56 m box of its own);
  * a FAST tile holds exactly one fast row -- planar v = (5, 0.125, 0), 3-D v = (0.1875, 0.03125, 6) -- and otherwise rows of at most
    0.25 m/s (3-D: 0.1875); a SLOW tile holds only such rows;
  * the fast row stands in the column of its box that faces a slow tile, its PARTNER -- v = (-0.25, 0, 0), 3-D (-0.125, 0, 0) -- in
    the facing column of that tile, GAP = 30 m (3-D: 20 m) away: between the reach without the fast row (19.9 m, 3-D 17.4 m, + 0.9 m
    with radii) and the true reach (114.5 m, 3-D 132 m).  The small lateral velocity keeps theta off 0.  The partner's whole
    pedestrian force is the fast row's term, so a dropped tile pair is the whole force of that row;
  * a pair never has a fast row on both sides: it could not show which tile's bound was wrong.

Two layouts.  'units' (uploaded with SFM_REORDER=0: the device's tiles are the caller's): each designed pair of tiles alone on a
site of a 512 m lattice (each site 3 m higher in y than the last), the tile indices and the fast row's lane chosen freely.  'stacks' (uploaded WITH the spatial packing):
strips side by side in x, GAP apart, each a stack of tiles 24 m apart in y, rows of a tile in (y, x) order -- the sort-tile-
recursive packing (sort by x, strips of strip_rows rows, each sorted by y) then leaves exactly these tiles whatever the caller's
order, which ``packing`` restates and the host file asserts; a strip holds at most ONE fast tile where its strip bound is at stake.

Carried bounds (the epilogue leaves the next tick's): 'starters' -- the fast rows stand at rest, target speed 6 m/s, and one tick of
0.4 s of the acceleration force brings them to 4.8 m/s, under the cap of 7.8 -- and 'carry3', a 3-D crowd whose fast rows have a target
speed of 8 m/s, so that an integrating tick does not cap their v_z.

``restate(crowd)`` states the rule of section 3.5 in float64 from the crowd's coordinates alone: the tiles' boxes, the largest
and second-largest speed of each tile, the gap between two boxes, the reach.
"""
import functools
from dataclasses import dataclass

import numpy as np

import _encounters as E
from carla_social_force_model_amd import scenarios

_f32 = scenarios._f32
STOCK = E.STOCK
PITCH, GRID, WAVE = 8.0, 8, 64
SIDE = PITCH * (GRID - 1)                     # 56 m: a tile's box
STACK = SIDE + 24.0                           # y pitch of stacked tiles: 24 m apart, beyond the reach of two slow tiles (20.8 m)
SITE = 512.0                                  # 'units': one designed pair of tiles per site
SITE_RISE = 3.0                               # ... each 3 m higher in y than the last: no two sites share a row's y (see ``build``)
GAP = {False: 30.0, True: 20.0}               # [3-D]
V_FAST = {False: (5.0, 0.125, 0.0), True: (0.1875, 0.03125, 6.0)}
V_PARTNER = {False: (-0.25, 0.0, 0.0), True: (-0.125, 0.0, 0.0)}
SLOW = {False: 0.25, True: 0.1875}            # largest speed of every other row
ROW = 3                                       # grid row of the fast row and of its partner
R_MAX = E.R_MAX
MARGIN = 0.01                                 # the gap clears every reach by 1 %
TERM_FACTOR = 1000.0                          # partner's term / the row's whole check_force allowance
# carried bounds: starters at rest, brought to ~4.8 m/s by the acceleration force within one tick of DT_CARRY
DT_CARRY, STARTER_SPEED, GAP_CARRY = 0.4, 6.0, 32.0
# a 3-D crowd carried one tick on: the cap (1.3 x 8 m/s) above the fast rows' 6 m/s; within dt = 2^-7 v_z decays by dt / tau = 1.6 % and
# the acceleration force adds 0.12 m/s in the plane, so the planar speed alone still does not reach the partner
DT_CARRY_3D, CAP_FREE_SPEED = 0.0078125, 8.0


# ---- the rule of DESIGN.md 3.5, float64 ---------------------------------------------------------------------------------------------------
def reach(va, vb, rad, r_max, p=STOCK):
    return p.gamma * 41.0 * np.log(2.0) * 1.001 * (1.0 + p.lam * (va + vb)) + (2.0 * r_max * 1.001 if rad else 0.0)


def box_gap(a, b):
    """Distance between two boxes (x0, y0, x1, y1)."""
    gx = max(0.0, a[0] - b[2], b[0] - a[2])
    gy = max(0.0, a[1] - b[3], b[1] - a[3])
    return float(np.hypot(gx, gy))


def packing(loc):
    """The sort-tile-recursive packing of an upload, restated: device row -> caller index, and tiles per strip.
    Sort by x; about sqrt(tiles * aspect) strips, aspect = x extent / y extent held to [1/64, 64]; each strip sorted by y; both
    sorts stable."""
    n = len(loc)
    x, y = np.float32(loc[:, 0]), np.float32(loc[:, 1])
    n_t = (n + WAVE - 1) // WAVE
    ex, ey = float(x.max() - x.min()), float(y.max() - y.min())
    aspect = min(max(ex / ey if ex > 0 and ey > 0 else 1.0, 1.0 / 64.0), 64.0)
    n_strips = max(1, min(n_t, int(np.floor(np.sqrt(n_t * aspect) + 0.5))))
    tps = (n_t + n_strips - 1) // n_strips
    order = np.argsort(x, kind="stable")
    for q in range(0, n, tps * WAVE):
        seg = order[q:q + tps * WAVE]
        order[q:q + tps * WAVE] = seg[np.argsort(y[seg], kind="stable")]
    return order, tps


@dataclass
class Restated:
    order: np.ndarray          # device row -> caller index
    tps: int                   # tiles per strip (1: no strips to speak of)
    box: np.ndarray            # (n_t, 4)
    vmax: np.ndarray           # (n_t,) largest speed of the tile (three components in a 3-D crowd)
    v2nd: np.ndarray           # (n_t,) second largest
    vmax_planar: np.ndarray    # (n_t,) largest speed from v_x, v_y alone
    r_max: float

    def strip_of(self, t):
        return t // self.tps

    def strip_tiles(self, s):
        return range(s * self.tps, min(len(self.box), (s + 1) * self.tps))

    def strip_box(self, s):
        b = self.box[list(self.strip_tiles(s))]
        return np.array([b[:, 0].min(), b[:, 1].min(), b[:, 2].max(), b[:, 3].max()])


def restate_state(loc, vel, radius, packed, z3):
    n = len(loc)
    order, tps = packing(loc) if packed else (np.arange(n), 1)
    n_t = (n + WAVE - 1) // WAVE
    box, vmax, v2nd, vpl = np.zeros((n_t, 4)), np.zeros(n_t), np.zeros(n_t), np.zeros(n_t)
    for t in range(n_t):
        rows = order[t * WAVE:(t + 1) * WAVE]
        p = loc[rows]
        box[t] = (p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max())
        sp = np.sort(np.linalg.norm(vel[rows] if z3 else vel[rows, :2], axis=1))
        vmax[t], v2nd[t] = sp[-1], sp[-2]
        vpl[t] = np.linalg.norm(vel[rows, :2], axis=1).max()
    return Restated(order, tps, box, vmax, v2nd, vpl, float(np.max(radius)))


def restate(crowd):
    return restate_state(crowd.sc.loc, crowd.sc.vel, crowd.sc.radius, crowd.spec.packed, crowd.spec.z3)


# ---- the crowds -----------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Spec:
    name: str
    layout: str                # 'units' | 'stacks'
    n: int
    z3: bool
    pairs: tuple               # ((fast tile, slow tile, lane of the fast row, lane of the partner), ...); 'stacks': lanes are the slots
    shape: tuple = ()          # 'stacks': (strips, tiles per strip)
    shuffled: bool = False     # rows handed over in a shuffled caller order
    starters: bool = False     # the fast rows start at rest and are brought up to speed by the acceleration force (carried bounds)
    cap_free: bool = False     # the fast rows' target speed is CAP_FREE_SPEED: an integrating tick does not cap them

    @property
    def packed(self):
        return self.layout == "stacks"


@dataclass
class Crowd:
    spec: Spec
    sc: scenarios.Scenario
    partner: np.ndarray        # (n,) caller index of the designed partner, -1
    pair: np.ndarray           # (n,) designed pair, -1
    side: np.ndarray           # (n,) 0 = the fast row, 1 = its partner
    designed: dict             # the B = 0 labels of ``_encounters``: none here
    n_pairs: int
    fast: np.ndarray           # (pairs,) caller index of the fast row
    slow: np.ndarray           # (pairs,) caller index of its partner
    tiles: np.ndarray          # (pairs, 2) device tile of the fast row, of the partner

    @property
    def paired(self):
        return self.partner >= 0


def _tile_origins(spec):
    """Box origin of every tile, and per designed pair the side (+1: the partner's tile lies towards +x)."""
    n_t = (spec.n + WAVE - 1) // WAVE
    org = np.zeros((n_t, 2))
    gap = GAP_CARRY if spec.starters else GAP[spec.z3]
    side = []
    if spec.layout == "units":
        seen = set()
        for k, (f, s, _, _) in enumerate(spec.pairs):
            sd = 1 if k % 2 == 0 else -1
            lo, hi = (f, s) if sd > 0 else (s, f)
            org[lo], org[hi] = (k * SITE, k * SITE_RISE), (k * SITE + SIDE + gap, k * SITE_RISE)
            side.append(sd)
            seen |= {f, s}
        for j, t in enumerate(sorted(set(range(n_t)) - seen)):
            org[t] = ((len(spec.pairs) + j) * SITE, (len(spec.pairs) + j) * SITE_RISE)
    else:
        strips, tps = spec.shape
        assert strips * tps == n_t
        for t in range(n_t):
            org[t] = ((t // tps) * (SIDE + gap), (t % tps) * STACK)
        for f, s, _, _ in spec.pairs:
            assert f % tps == s % tps and abs(f // tps - s // tps) == 1, (spec.name, f, s)
            side.append(1 if s > f else -1)
    return org, side


@functools.lru_cache(maxsize=None)
def build(spec):
    rng = np.random.default_rng(7100 + sum(map(ord, spec.name)))
    n, z3 = spec.n, spec.z3
    n_t = (n + WAVE - 1) // WAVE
    org, sides = _tile_origins(spec)
    # slot of lane l in tile t: (l + rot[t]) % 64 -- 'units' turn the grid so that the designed row gets the lane asked for
    rot = np.zeros(n_t, dtype=np.int64)
    fast_slot = {+1: ROW * GRID + GRID - 1, -1: ROW * GRID}
    fast, slow = [], []
    for (f, s, lf, ls), sd in zip(spec.pairs, sides):
        if spec.packed:
            lf, ls = fast_slot[sd], fast_slot[-sd]
        rot[f], rot[s] = fast_slot[sd] - lf, fast_slot[-sd] - ls
        fast.append(f * WAVE + lf)
        slow.append(s * WAVE + ls)
    assert max(fast + slow) < n, (spec.name, max(fast + slow), n)
    rows = np.arange(n)
    slot = (rows % WAVE + rot[rows // WAVE]) % WAVE
    loc = np.zeros((n, 3))
    loc[:, 0], loc[:, 1] = org[rows // WAVE, 0] + PITCH * (slot % GRID), org[rows // WAVE, 1] + PITCH * (slot // GRID)
    lim = 11 if not z3 else 7                                  # / 64 per component: norm <= 0.243 (3-D with v_z <= 2 / 64: 0.158), + 0.003
    vel = np.zeros((n, 3))
    vel[:, :2] = rng.integers(-lim, lim + 1, (n, 2)) / 64.0
    vel[(vel[:, 0] == 0) & (vel[:, 1] == 0), 0] = 1.0 / 64.0
    # ... and off the 1 / 64 lattice by up to 1 / 512 a component, every row its own way: rows on a lattice of positions with a lattice
    # of velocities meet at theta = 0 exactly -- a row dead ahead with D_y = 0 -- which is an exposure on the row (1e-59 m/s^2 from
    # another site, 5e-4 within a tile), and a shard decides BOTH rows of a designed pair on their own.  (Designed rows: SITE_RISE.)
    vel[:, 0] += ((rows * 0.9068996821171) % 1.0 - 0.5) / 256.0
    vel[:, 1] += ((rows * 0.2915026221292) % 1.0 - 0.5) / 256.0
    if z3:
        vel[:, 2] = rng.integers(-2, 3, n) / 64.0
        loc[:, 2] = rng.integers(0, 4, n) * 0.5
    rad = _f32(rng.uniform(0.2, R_MAX, n))
    rad[rng.integers(0, n)] = float(np.float32(R_MAX))
    speed = np.linalg.norm(vel[:, :2], axis=1)
    wp = loc + 64.0 * vel
    ts = speed.copy()
    for (i, j), sd in zip(zip(fast, slow), sides):
        vel[i], vel[j] = np.array(V_FAST[z3]) * (sd, 1, 1), np.array(V_PARTNER[z3]) * (sd, 1, 1)
        loc[i, 2] = loc[j, 2] = 0.0
        for r in (i, j):
            wp[r], ts[r] = loc[r] + 64.0 * vel[r], np.linalg.norm(vel[r, :2])
        if spec.starters:                                   # at rest, heading for the partner a little off the axis
            vel[i] = 0.0
            wp[i], ts[i] = loc[i] + np.array([64.0 * sd, 1.625, 0.0]), STARTER_SPEED
        if spec.cap_free:                                   # a target speed whose cap (1.3 x) lies above the fast row's 6 m/s
            ts[i] = CAP_FREE_SPEED
    wp[:, 2] = 0.0
    partner, pair, side = np.full(n, -1), np.full(n, -1), np.zeros(n, dtype=np.int64)
    for k, (i, j) in enumerate(zip(fast, slow)):
        partner[i], partner[j], pair[i], pair[j], side[j] = j, i, k, k, 1
    fast, slow = np.array(fast), np.array(slow)
    tiles = np.stack([fast // WAVE, slow // WAVE], axis=1)
    loc, vel, wp, ts = _f32(loc), _f32(vel), _f32(wp), _f32(ts)
    if spec.shuffled:
        perm = rng.permutation(n)                          # caller row c holds designed row perm[c]
        inv = np.argsort(perm)
        loc, vel, wp, ts, rad, pair, side = loc[perm], vel[perm], wp[perm], ts[perm], rad[perm], pair[perm], side[perm]
        partner = np.where(partner[perm] >= 0, inv[np.maximum(partner[perm], 0)], -1)
        fast, slow = inv[fast], inv[slow]
    sc = scenarios.Scenario(loc=loc, vel=vel, waypoint=wp, target_speed=ts, radius=rad, mode=np.ones(n, dtype=np.int64),
                            world_side=float(np.float32(loc[:, :2].max() + SITE)), seed=7100)
    return Crowd(spec, sc, partner, pair, side, {}, len(fast), fast, slow, tiles)


def moved(crowd, loc, vel):
    """``crowd`` with another state (the carried-bounds cell: after its first tick)."""
    import copy
    out = copy.copy(crowd)
    out.sc = copy.copy(crowd.sc)
    out.sc.loc, out.sc.vel = np.asarray(loc, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    return out


# 'units', 8 tiles: fast first (0), middle (1, 4), last (7); the partner's tile above / below, and within / beyond n_t / 2 ahead of the
# fast tile (the list keeps a pair under the tile from which the other is at most n_t / 2 ahead)
_A = ((0, 5, 0, 40), (1, 6, 1, 63), (7, 2, 31, 0), (4, 3, 32, 17))
_B = ((5, 0, 63, 9), (6, 1, 32, 31), (2, 7, 31, 32), (3, 4, 1, 62))          # the roles exchanged: every tile is the fast one somewhere
_R = ((8, 3, 16, 5), (0, 5, 63, 1), (1, 6, 0, 33), (7, 2, 32, 60))          # N = 64 * 8 + 17: the fast row at the last index
# sharded ranks (below): four disjoint pairs of tiles whose partner lies 2 above / 6 above / 1 below / 5 below the fast tile -- with the
# fast tile on one rank and the partner on another that is every direction (remote tile below / above the own one) and distance
# (within / beyond n_t / 2 ahead of it) on both ranks -- the four lanes dealt over them as a Latin square
_LANES, _TYPES, _PARTNER_LANES = (0, 31, 32, 63), ((1, 3), (0, 6), (5, 4), (7, 2)), (40, 9, 0, 63)
_S = tuple(tuple((f, s, _LANES[(j + k) % 4], _PARTNER_LANES[(j + k) % 4]) for j, (f, s) in enumerate(_TYPES)) for k in range(4))
# ragged bounds: a cut at row 200 goes through tile 3 (lanes 0-7 | 8-63), cuts at rows 100 and 300 through tiles 1 (lanes 0-35 | 36-63)
# and 4 (0-43 | 44-63); the fast row of a cut tile on the side of the rank that owns the partner, or on the other rank's
_C2A = ((3, 6, 0, 40), (0, 1, 31, 9), (7, 5, 32, 0), (4, 2, 63, 17))
_C2B = ((3, 6, 63, 40), (0, 1, 32, 9), (7, 5, 0, 0), (4, 2, 31, 17))
_C3 = ((1, 2, 63, 5), (4, 7, 0, 33), (0, 6, 32, 60), (5, 3, 31, 1))
SPECS = {s.name: s for s in (
    Spec("s0", "units", 512, False, _S[0]), Spec("s1", "units", 512, False, _S[1]), Spec("s2", "units", 512, False, _S[2]),
    Spec("s3", "units", 512, False, _S[3]), Spec("s0z", "units", 512, True, _S[0]), Spec("s1z", "units", 512, True, _S[1]),
    Spec("s2z", "units", 512, True, _S[2]), Spec("s3z", "units", 512, True, _S[3]),
    Spec("c2a", "units", 512, False, _C2A), Spec("c2bz", "units", 512, True, _C2B), Spec("c3", "units", 512, False, _C3),
    Spec("c3z", "units", 512, True, _C3),
    Spec("a", "units", 512, False, _A), Spec("b", "units", 512, False, _B), Spec("ragged", "units", 529, False, _R),
    Spec("a3", "units", 512, True, _A), Spec("b3", "units", 512, True, _B), Spec("ragged3", "units", 529, True, _R),
    # 'stacks', 2 strips of 16 tiles (cross-strip pairs are listed under the tile of strip 0: strip 1's bound is the one at stake, and
    # strip 1 holds ONE fast tile): in the middle of its strip / the strip's last tile, the sixteenth wave's share of the merged launch
    Spec("strip-mid", "stacks", 2048, False, ((21, 5, 0, 0), (2, 18, 0, 0), (9, 25, 0, 0)), (2, 16)),
    Spec("strip-w15", "stacks", 2048, False, ((31, 15, 0, 0), (3, 19, 0, 0)), (2, 16)),
    Spec("strip-mid3", "stacks", 2048, True, ((21, 5, 0, 0), (2, 18, 0, 0), (9, 25, 0, 0)), (2, 16)),
    Spec("strip-w153", "stacks", 2048, True, ((31, 15, 0, 0), (3, 19, 0, 0)), (2, 16)),
    # as shipped: 5 strips of 13 tiles, shuffled caller order, above the automatic cutoff's 4096
    Spec("shipped", "stacks", 4160, False, ((0, 13, 0, 0), (32, 19, 0, 0), (64, 51, 0, 0), (43, 56, 0, 0)), (5, 13), shuffled=True),
    Spec("starters", "units", 512, False, _A, starters=True), Spec("carry3", "units", 512, True, _B, cap_free=True),
)}


def crowd(name):
    return build(SPECS[name])


# ---- the cells both files read ----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Cell:
    kind: str                  # 'sym' | 'ordered' | 'carried' | 'shipped'
    crowd: str
    rad: bool
    env: tuple                 # ((knob, value), ...)

    @property
    def id(self):
        knobs = "-".join(f"{k[4:].lower()}{v}" for k, v in self.env if k not in ("SFM_SYM", "SFM_CUTOFF", "SFM_FUSED"))
        return f"{self.kind}-{self.crowd}-{'rad' if self.rad else 'norad'}" + (f"-{knobs}" if knobs else "")


def _sym(crowd_, rad, strips):
    reorder = 1 if SPECS[crowd_].packed else 0
    return Cell("sym", crowd_, rad, (("SFM_SYM", 1), ("SFM_CUTOFF", 1), ("SFM_FUSED", 0), ("SFM_REORDER", reorder), ("SFM_STRIPS", strips)))


def _ordered(crowd_, rad, ipw, team):
    return Cell("ordered", crowd_, rad, (("SFM_SYM", 0), ("SFM_CUTOFF", 1), ("SFM_REORDER", 0), ("SFM_IPW", ipw), ("SFM_TEAM", team)))


CELLS = ([_sym(c, rad, 0) for c in ("a", "b", "ragged", "a3", "b3", "ragged3") for rad in (False, True)]
         + [_sym(c, rad, 1) for c in ("strip-mid", "strip-w15", "strip-mid3", "strip-w153") for rad in (False, True)]
         + [_ordered("a", False, 8, 4), _ordered("b", True, 8, 4), _ordered("a3", True, 8, 4), _ordered("b3", False, 8, 4),
            _ordered("b", False, 1, 1), _ordered("a", True, 1, 1), _ordered("b3", True, 1, 1), _ordered("a3", False, 1, 1)]
         + [Cell("carried", c, rad, (("SFM_SYM", 1), ("SFM_CUTOFF", 1), ("SFM_FUSED", 0), ("SFM_REORDER", 0), ("SFM_STRIPS", 0)))
            for c, rad in (("starters", True), ("carry3", False))]
         + [Cell("shipped", "shipped", True, ())])
PED_ONLY = E.PED_ONLY
CARRY_FORCES = ("acceleration_force", "pedestrian_force")


def carry_dt(spec):
    """Step length of a carried-bounds cell."""
    return DT_CARRY if spec.starters else DT_CARRY_3D


# ---- sharded ranks (tests/test_speed_bound_shards_host.py, tests/test_speed_bound_shards_gpu.py) -----------------------------------------------
# A rank owns the device rows [bounds[r], bounds[r + 1]).  ROLE of a rank in a designed pair, by the rows it owns:
#   'oo'               it owns the fast row and its partner: one decision serves both ends, as in a whole crowd;
#   'fo' + dir + dist  it owns the FAST row, the partner is another rank's: it decides the fast row's end alone (one-sided);
#   'fr' + dir + dist  the fast row is another rank's (its tile's speed comes from rows that arrived by the exchange), it owns the
#                      PARTNER and decides the partner's end alone;
#   dir  '+' / '-'     the remote row's tile index lies above / below the own row's,
#   dist 'w' / 'b'     within / beyond n_t / 2 ahead of it (2 ((remote - own) mod n_t) < n_t).
# Every role must occur with the fast row at lanes 0, 31, 32 and 63 over the cells (the host file asserts it).
ONE_SIDED = tuple(k + d + w for k in ("fo", "fr") for d in "+-" for w in "wb")
ROLES = ("oo",) + ONE_SIDED
ROLE_LANES = (0, 31, 32, 63)


@dataclass(frozen=True)
class ShardSpec:
    crowd: str
    world: int
    bounds: tuple              # row bounds of the ranks, bounds[0] = 0, bounds[world] = N
    roles: tuple               # per designed pair: ((rank, role), ...) of the one or two ranks that own one of its rows
    cut: tuple = ()            # ragged bounds, per designed pair: the fast TILE is cut by a bound and the rank that owns the partner owns rows
    #                            of it -- 'own': the fast row among them, 'other': the fast row is the other rank's; '': neither
    partition: tuple = ()      # (gx, gy) rank blocks (sfm_set_partition); (): the plain packing of an upload
    tag: str = ""

    @property
    def name(self):
        return f"{self.crowd}-w{self.world}{self.tag}"

    @property
    def aligned(self):
        return all(b % WAVE == 0 for b in self.bounds[:-1])


def _eq(n, world):
    return tuple(n * k // world // WAVE * WAVE for k in range(world)) + (n,)


_ROLES_S = {       # the pairs of _TYPES: (1, 3), (0, 6), (5, 4), (7, 2)
    2: ((((0, "oo"),), ((0, "fo+b"), (1, "fr-w")), ((1, "oo"),), ((0, "fr+b"), (1, "fo-w")))),
    4: ((((0, "fo+w"), (1, "fr-b")), ((0, "fo+b"), (3, "fr-w")), ((2, "oo"),), ((1, "fr+b"), (3, "fo-w")))),
    8: ((((1, "fo+w"), (3, "fr-b")), ((0, "fo+b"), (6, "fr-w")), ((4, "fr+w"), (5, "fo-b")), ((2, "fr+b"), (7, "fo-w")))),
}
_ROLES_R = {       # _R: (8, 3), (0, 5), (1, 6), (7, 2) at N = 529, nine tiles
    2: ((0, 256, 529), (((0, "fr+b"), (1, "fo-w")), ((0, "fo+b"), (1, "fr-w")), ((0, "fo+b"), (1, "fr-w")), ((0, "fr+b"), (1, "fo-w")))),
    4: ((0, 128, 256, 384, 529), (((1, "fr+b"), (3, "fo-w")), ((0, "fo+b"), (2, "fr-w")), ((0, "fo+b"), (3, "fr-w")), ((1, "fr+b"), (3, "fo-w")))),
    8: ((0, 64, 128, 192, 256, 320, 384, 448, 529),
        (((3, "fr+b"), (7, "fo-w")), ((0, "fo+b"), (5, "fr-w")), ((1, "fo+b"), (6, "fr-w")), ((2, "fr+b"), (7, "fo-w")))),
}
_ROLES_A = {       # _A: (0, 5), (1, 6), (7, 2), (4, 3)
    2: (((0, "fo+b"), (1, "fr-w")), ((0, "fo+b"), (1, "fr-w")), ((0, "fr+b"), (1, "fo-w")), ((0, "fr+w"), (1, "fo-b"))),
    4: (((0, "fo+b"), (2, "fr-w")), ((0, "fo+b"), (3, "fr-w")), ((1, "fr+b"), (3, "fo-w")), ((1, "fr+w"), (2, "fo-b"))),
}
_ROLES_B = {       # _B: (5, 0), (6, 1), (2, 7), (3, 4)
    2: (((0, "fr+b"), (1, "fo-w")), ((0, "fr+b"), (1, "fo-w")), ((0, "fo+b"), (1, "fr-w")), ((0, "fo+w"), (1, "fr-b"))),
    4: (((0, "fr+b"), (2, "fo-w")), ((0, "fr+b"), (3, "fo-w")), ((1, "fo+b"), (3, "fr-w")), ((1, "fo+w"), (2, "fr-b"))),
}
_ROLES_C3 = (((1, "oo"),), ((1, "fo+w"), (2, "fr-b")), ((0, "fo+b"), (2, "fr-w")), ((1, "fr+w"), (2, "fo-b")))
_ROLES_MID = {     # two strips of sixteen tiles: a pair's tiles are n_t / 2 apart
    2: (((0, "fr+b"), (1, "fo-b")), ((0, "fo+b"), (1, "fr-b")), ((0, "fo+b"), (1, "fr-b"))),
    4: (((0, "fr+b"), (2, "fo-b")), ((0, "fo+b"), (2, "fr-b")), ((1, "fo+b"), (3, "fr-b"))),
}
_ROLES_W15 = {
    2: (((0, "fr+b"), (1, "fo-b")), ((0, "fo+b"), (1, "fr-b"))),
    4: (((1, "fr+b"), (3, "fo-b")), ((0, "fo+b"), (2, "fr-b"))),
}
SHARDS = {s.name: s for s in (
    # units, whole tiles: 4 | 4, two each, one each (no own-own pair: every designed pair is one-sided on both ranks)
    [ShardSpec(c + z, w, _eq(512, w), _ROLES_S[w]) for c in ("s0", "s1", "s2", "s3") for z in ("", "z") for w in (2, 4, 8)]
    + [ShardSpec(c, w, *_ROLES_R[w]) for c in ("ragged", "ragged3") for w in (2, 4, 8)]
    + [ShardSpec("starters", w, _eq(512, w), _ROLES_A[w]) for w in (2, 4)] + [ShardSpec("carry3", w, _eq(512, w), _ROLES_B[w]) for w in (2, 4)]
    # units, ragged bounds: every rank takes the ordered kernel, whose keep mask then works on tiles it owns only part of
    + [ShardSpec("c2a", 2, (0, 200, 512), (((0, "fo+w"), (1, "fr-b")), ((0, "oo"),), ((1, "oo"),), ((0, "fr+w"), (1, "fo-b"))),
                 cut=("other", "", "", "")),
       ShardSpec("c2bz", 2, (0, 200, 512), (((1, "oo"),), ((0, "oo"),), ((1, "oo"),), ((0, "fr+w"), (1, "fo-b"))), cut=("own", "", "", "")),
       ShardSpec("c3", 3, (0, 100, 300, 512), _ROLES_C3, cut=("own", "other", "", "")),
       ShardSpec("c3z", 3, (0, 100, 300, 512), _ROLES_C3, cut=("own", "other", "", ""))]
    # stacks: one strip per rank (every cross-strip pair is remote on both sides), half a strip each
    + [ShardSpec(c + z, w, _eq(2048, w), r[w]) for c, r in (("strip-mid", _ROLES_MID), ("strip-w15", _ROLES_W15)) for z in ("", "3")
       for w in (2, 4)]
    # rank blocks: two columns by x of two blocks by y -- a block is half a strip, and the block packing leaves the designed tiles
    + [ShardSpec("strip-mid", 4, _eq(2048, 4), _ROLES_MID[4], partition=(2, 2), tag="-2x2")]
)}


@dataclass(frozen=True)
class ShardCell:
    kind: str                  # 'plain' | 'ragged' | 'split' | 'starters'
    shard: str
    rad: bool
    env: tuple
    split: bool = False        # the integrating tick as begin / exchange / end (else run(1))

    @property
    def spec(self):
        return SHARDS[self.shard]

    @property
    def id(self):
        knobs = "-".join(f"{k[4:].lower()}{v}" for k, v in self.env if k in ("SFM_STRIPS", "SFM_IPW", "SFM_TEAM"))
        return f"{self.kind}-{self.shard}-{'rad' if self.rad else 'norad'}" + (f"-{knobs}" if knobs else "") + ("-split" if self.split else "")


def _shard_env(crowd_, strips=0, **more):
    """SFM_SYM=1 throughout: a rank takes the ordered kernel because of its bounds, not because of a knob."""
    reorder = 1 if SPECS[crowd_].packed else 0
    return (("SFM_SYM", 1), ("SFM_CUTOFF", 1), ("SFM_FUSED", 0), ("SFM_REORDER", reorder), ("SFM_STRIPS", strips),
            ("SFM_RESORT_EVERY", 0)) + tuple(more.items())


def _plain(crowd_, world, rad, strips=0, tag=""):
    return ShardCell("plain", f"{crowd_}-w{world}{tag}", rad, _shard_env(crowd_, strips))


_STACKS = ("strip-mid", "strip-w15", "strip-mid3", "strip-w153")
SHARD_CELLS = (
    [_plain(c, 8, rad) for c, rad in (("s0", False), ("s1z", True), ("s2", True), ("s3z", False), ("ragged", False), ("ragged3", True))]
    + [_plain(c, 2, rad) for c, rad in (("s0z", False), ("s1", True), ("ragged", False), ("ragged3", True))]
    + [_plain(c, 4, rad) for c, rad in (("s2z", True), ("s3", False), ("ragged", True), ("ragged3", False))]
    + [ShardCell("ragged", f"{c}-w{w}", rad, _shard_env(c, SFM_IPW=ipw, SFM_TEAM=team))
       for c, w, rad, ipw, team in (("c2a", 2, False, 4, 1), ("c2bz", 2, True, 4, 1), ("c3", 3, True, 8, 4), ("c3z", 3, False, 8, 4))]
    + [_plain(c, w, (k + w // 2 + strips) % 2 == 1, strips) for k, c in enumerate(_STACKS) for w in (2, 4) for strips in (0, 1)]
    + [_plain("strip-mid", 4, True, 1, tag="-2x2")]
    + [ShardCell("split", s, rad, _shard_env(SHARDS[s].crowd, strips), split=True)
       for s, rad, strips in (("s0-w2", False, 0), ("s1z-w4", True, 0), ("strip-mid-w2", True, 1), ("strip-w153-w4", False, 1),
                              ("carry3-w2", True, 0), ("carry3-w4", False, 0))]
    + [ShardCell("starters", f"{c}-w{w}", rad, _shard_env(c), split=split)
       for c, rad in (("starters", True), ("carry3", False)) for w in (2, 4) for split in (False, True)]
)
# The integrating split-tick cells, dt = DT_SPLIT: the designed term moves the partner's v' by >= VELOCITY_FACTOR allowances of
# check_velocity (at dt = 0.05 by 40-60).  The allowance is 1e-5 |v'|, and the fast row's own |v'| is 20-40 times its partner's (5 m/s;
# in 3-D the cap, 1.3 x its planar target speed, takes the v_z off it and most of the term's effect with it): on the fast row's end the
# term moves v' by 25-60 allowances, held to VELOCITY_FACTOR_FAST -- a dropped end still misses check_velocity twentyfold -- and to
# VELOCITY_FACTOR in the 3-D crowd whose fast rows no cap touches, 'carry3'.
DT_SPLIT = DT_CARRY
VELOCITY_FACTOR, VELOCITY_FACTOR_FAST = 100.0, 20.0
