"""DESIGNED POLYLINES for the geometry forces (tests/test_geo_cases_host.py on the CPU, tests/test_geo_cases_gpu.py on the GPU; DESIGN.md
section 4).  NumPy only, no GPU code here.

Every other parity test that runs a border or an obstacle force adds the oracle's tie exposure (``_parity.geometry_tie_exposure`` /
``tie_rel``): the jump the reference makes when np.argmin picks another of two equally near points (forces.py:154,228) or a strict
``<`` cull flips (forces.py:149-150,222-223).  In random crowds exact ties do not occur, so the rule itself -- the FIRST of equally
near points, a centre exactly at the limit DROPPED -- is never asserted.  Here it is, with no exposure at all.

A CASE is one pedestrian and the few polylines it keeps, alone on a site of a 128 m lattice (thresholds 20 m and 50 m, section lengths
<= 16 m): the row's force of a kind IS the term of its own polyline(s).  EXACTNESS: inside a case every coordinate is a multiple of
1/16 m, site origins are multiples of 128 m, radii and velocities are dyadic, every squared distance a case decides on is below 2^13.
Then x - px, its square and fmaf(ax, ax, ay * ay) are exact in fp32 (at most 13 + 8 bits), the device's comparison IS the exact
comparison, and no exposure is owed.  ``crowd`` asserts this for every crowd it builds (``assert_exact``).

TIE MATERIAL: the twelve points at squared distance 25/16 -- (+-1.25, 0), (0, +-1.25), (+-1, +-0.75), (+-0.75, +-1).  Every other point
of a scanned polyline is a filler at squared distance >= 8; "one quantum nearer" moves the larger coordinate of a tie point 1/16 in.

Cases, per kind (border / static obstacle / dynamic obstacle) unless said otherwise:
  scan      polylines that fail sfm_set_borders' straight test, P in SCAN_P: a unique minimum at slot 0, 7, 8, 63, 64, P - 1; exact
            two-way ties inside a group of 8, across groups of a 64-point trip, across trips and at the tail; one three-way tie;
            near misses at (7, 8) and (63, 64) with the later / the earlier point one quantum nearer; the pedestrian ON a point.
  straight  (borders) uniformly sampled straight lines, P = 8, 9, 65, along x and oblique ((3, 4) / 4 or / 8 per step): the foot of the
            perpendicular exactly half way between samples k and k + 1 (k = 0 .. 3 and P - 2: k expected), beyond either end, and the
            pedestrian exactly on a sample (d = 0: stateutils.normalize's zero guard, the term is exactly 0).
  cull      the centre exactly at the limit (dropped), one quantum inside (kept), one quantum outside (dropped); the points stay at
            1.25 m, so a polyline kept by mistake shows as a term of 0.1 m/s^2.
  cross     two polylines whose nearest points are equally near (the observations' cross-polyline rule; for the forces: two terms).
Obstacle cases carry velocities that put the angle between e and t near +-0.5 rad with |D| = 3 (theta away from 0 and +-pi).

``crowd(n, order, seed, start, z3)`` lays cases start, start + 1, ... (cyclically) on n rows, one site per row; order "random" permutes
which case lands on which row and which polyline gets which index k (the index decides the finder's wave, run and slice).
``multi_crowd`` gives every row several kept polylines (the finder's list overflow).  ``reference`` is ``O.tick_forces`` with
``tie_rel=0.0``; ``expected_points`` is the designed nearest point of every (row, kind), from the slots alone.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import _parity as P
from _encounters import QUALIFY_TERM                     # noqa: F401  (1e-3 m/s^2: the host file's floor for a kept term)
from oracle import sfm_oracle as O

Q = 1.0 / 16.0
SITE = 128.0
SITE_W = 16                    # sites per lattice row
RADIUS = 0.25
TARGET_SPEED = 1.25
KINDS = ("border", "static", "dynamic")
FORCE_OF_KIND = ("border_force", "static_obstacle_force", "dynamic_obstacle_force")
D2_LIMIT = 2.0 ** 13
TIE_D2 = 25.0 / 16.0
# counter-clockwise from +x; the gaps alternate 36.87 and 16.26 degrees
TIE = np.array([(1.25, 0.0), (1.0, 0.75), (0.75, 1.0), (0.0, 1.25), (-0.75, 1.0), (-1.0, 0.75), (-1.25, 0.0), (-1.0, -0.75),
                (-0.75, -1.0), (0.0, -1.25), (0.75, -1.0), (1.0, -0.75)])
SCAN_P = (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200)
UNIQUE_SLOTS = (0, 7, 8, 63, 64)
# (slots tied, the earliest expected) -> the polyline lengths the tie is built at
TIES = {(0, 1): (2, 200), (0, 7): (8, 65), (3, 5): (7, 128), (7, 8): (9, 200), (0, 8): (9, 129), (5, 58): (63, 127), (63, 64): (65, 200),
        (0, 64): (65, 128), (5, 130): (200,), (71, 72): (127, 200), (127, 128): (129,), (2, 9, 70): (127, 200)}
NEAR = {(7, 8): (9, 200), (63, 64): (65, 200)}
SECTION_LENGTH = (8.0, 16.0, 4.0)
PED_VEL = np.array([(0.5, 0.25), (-0.25, 0.75), (0.75, -0.5), (-0.5, -0.25)])
OBS_VEL = np.array([(1.0, 0.5), (-0.75, 1.0), (0.5, -1.0), (-1.0, -0.5)])
PED_OFF = np.array([(0.0, 0.0), (3 * Q, -2 * Q), (-5 * Q, 1.0), (2.0, 7 * Q)])      # where on its site a pedestrian stands


@dataclass
class Poly:
    kind: int                           # 0 border, 1 static obstacle, 2 dynamic obstacle
    pts: np.ndarray                     # (P, 2) offsets from the pedestrian
    center: np.ndarray                  # (2,) offset from the pedestrian: an input of its own (forces.py:127-132, 285-288)
    length: float = 8.0                 # borders: section_length
    exp: int = 0                        # slot of the expected nearest point
    alts: tuple = ()                    # tie: the later slots at the same distance; otherwise the runner-up slot
    tie: bool = False
    kept: bool = True                   # does the reference's cull keep it?
    dv: np.ndarray = None               # obstacles: v_pedestrian - v_obstacle
    obs_vel: np.ndarray = None          # dynamic obstacles, set by ``_case``
    straight: bool = False              # built to pass sfm_set_borders' straight test


@dataclass
class Case:
    name: str
    polys: list
    ped_vel: np.ndarray
    zero_term: bool = False             # the pedestrian stands ON a border point: the term is exactly 0 (stateutils.normalize)
    tags: tuple = ()


def _round_q(v):
    return np.round(np.asarray(v, dtype=np.float64) / Q) * Q


def _dv_for(point, phi, Dn=3.0, lam=2.0):
    """A dyadic relative velocity that puts the angle between e (towards ``point``) and t = D / |D| near ``phi`` with |D| near Dn."""
    d = float(np.hypot(*point))
    e = point / d if d > 0 else np.zeros(2)
    beta = float(np.arctan2(point[1], point[0])) if d > 0 else 0.0
    D = Dn * np.array([np.cos(beta - phi), np.sin(beta - phi)])
    return _round_q((D - e) / lam)


def _filler(j, sx, sy):
    """Distinct points at squared distance >= 8 that lie on no straight line."""
    return np.array([sx * (2.0 + 0.25 * (j % 40)), sy * (2.0 + 0.5 * (j // 40) + Q * ((j * j) % 3))])


def _scan_pts(n_pts, placed, cnt):
    sx, sy = (1.0, -1.0)[cnt & 1], (1.0, -1.0)[(cnt >> 1) & 1]
    pts = np.array([_filler(j, sx, sy) for j in range(n_pts)]).reshape(n_pts, 2)
    for slot, p in placed.items():
        pts[slot] = p
    return pts


def _nearer(p):
    """One quantum nearer: the larger coordinate moves 1/16 towards the pedestrian."""
    p = np.array(p, dtype=np.float64)
    c = int(np.argmax(np.abs(p)))
    p[c] -= np.sign(p[c]) * Q
    return p


def _poly(kind, pts, exp, alts, tie, cnt, phi=None, **kw):
    center = np.array([(3 * Q, -2 * Q), (1.0, 1.0), (-2.0, 0.5)][cnt % 3])
    pl = Poly(kind, pts, kw.pop("center", center), kw.pop("length", SECTION_LENGTH[cnt % 2]), exp, tuple(alts), tie, **kw)
    if kind:
        pl.dv = _dv_for(pts[exp], (0.5, -0.5)[cnt & 1] if phi is None else phi)
    return pl


def _case(name, polys, cnt, ped_vel=None, zero_term=False, tags=()):
    statics = [p for p in polys if p.kind == 1]
    dynamics = [p for p in polys if p.kind == 2]
    if ped_vel is None:
        ped_vel = statics[0].dv if statics else dynamics[0].dv + OBS_VEL[cnt % 4] if dynamics else PED_VEL[cnt % 4]
    for p in dynamics:
        p.obs_vel = ped_vel - p.dv
    for p in statics:
        p.dv = np.array(ped_vel, dtype=np.float64)              # a static obstacle is at rest (forces.py:212-213): dv is the row's velocity
    return Case(name, polys, np.array(ped_vel, dtype=np.float64), zero_term, tuple(tags))


def _scan_cases(kind):
    out, kn = [], KINDS[kind]
    cnt = 7 * kind
    for n_pts in SCAN_P:
        for slot in sorted({s for s in UNIQUE_SLOTS if s < n_pts} | {n_pts - 1}):
            pts = _scan_pts(n_pts, {slot: TIE[cnt % 12]}, cnt)
            alt = int(np.argmin(np.where(np.arange(n_pts) == slot, np.inf, np.sum(pts * pts, axis=1)))) if n_pts > 1 else None
            out.append(_case(f"{kn}-scan-P{n_pts}-min{slot}", [_poly(kind, pts, slot, () if alt is None else (alt,), False, cnt)], cnt,
                             tags=("scan", "unique")))
            cnt += 1
    for slots, lengths in TIES.items():
        for n_pts in lengths:
            m = [(cnt + q * (1 + cnt % 5)) % 12 for q in range(len(slots))]
            assert len(set(m)) == len(m), (slots, m)
            pts = _scan_pts(n_pts, {s: TIE[q] for s, q in zip(slots, m)}, cnt)
            out.append(_case(f"{kn}-scan-P{n_pts}-tie{'_'.join(map(str, slots))}", [_poly(kind, pts, slots[0], slots[1:], True, cnt)], cnt,
                             tags=("scan", "tie")))
            cnt += 1
    for (a, b), lengths in NEAR.items():
        for n_pts in lengths:
            for who, exp, other in (("later", b, a), ("earlier", a, b)):
                m0, m1 = cnt % 12, (cnt + 5) % 12
                pts = _scan_pts(n_pts, {exp: _nearer(TIE[m0]), other: TIE[m1]}, cnt)
                out.append(_case(f"{kn}-scan-P{n_pts}-near{a}_{b}-{who}", [_poly(kind, pts, exp, (other,), False, cnt)], cnt,
                                 tags=("scan", "near")))
                cnt += 1
    # the pedestrian exactly ON point 3 of 9 (d = 0): a border's term is exactly 0; an obstacle's is finite in the oracle (e = 0,
    # np.arctan2(0, 0) = 0, -0 / B = -0), so the case stays for all three kinds
    pts = _scan_pts(9, {3: np.zeros(2)}, cnt)
    out.append(_case(f"{kn}-scan-P9-on3", [_poly(kind, pts, 3, (int(np.argmin(np.where(np.arange(9) == 3, np.inf, np.sum(pts * pts, axis=1)))),),
                                                 False, cnt, phi=0.5)], cnt, zero_term=kind == 0, tags=("scan", "on")))
    return out


def _line(n_pts, step, first):
    return first[None, :] + np.arange(n_pts)[:, None] * step[None, :]


def _straight_cases():
    """Borders only: the shortcut of geo_item is for borders.  ``foot`` is where the perpendicular meets the line, in steps from
    sample 0; the pedestrian stands |normal| off the line."""
    out, cnt = [], 100
    for n_pts in (8, 9, 65):
        for tag, step, normal in (("x", np.array([0.5, 0.0]), np.array([0.0, -1.0])),
                                  ("oblique", np.array([3.0, 4.0]) / (8.0 if n_pts == 65 else 4.0), np.array([-1.0, 0.75]))):
            feet = [(f"half{k}", k + 0.5, k, (k + 1,), True) for k in (0, 1, 2, 3, n_pts - 2)]
            feet += [("before", -1.5, 0, (1,), False), ("after", n_pts + 0.5, n_pts - 1, (n_pts - 2,), False)]
            for what, foot, exp, alts, tie in feet:
                pts = _line(n_pts, step, normal - foot * step)
                pl = Poly(0, pts, pts[exp].copy(), 16.0, exp, alts, tie, straight=True)
                out.append(_case(f"border-straight-{tag}-P{n_pts}-{what}", [pl], cnt, tags=("straight",)))
                cnt += 1
            pts = _line(n_pts, step, -3.0 * step)                                  # exactly on sample 3
            out.append(_case(f"border-straight-{tag}-P{n_pts}-on3", [Poly(0, pts, pts[3].copy(), 16.0, 3, (2,), False, straight=True)], cnt,
                             zero_term=True, tags=("straight", "on")))
            cnt += 1
    return out


CULL = ((np.array([3.0, 4.0]), 5.0), (np.array([12.0, 16.0]), 20.0), (np.array([30.0, 40.0]), 50.0))     # centre offset, limit (stock)


def _cull_cases():
    out, cnt = [], 200
    for kind, (c, limit) in enumerate(CULL):
        for what, dy, kept in (("at", 0.0, False), ("inside", -Q, True), ("outside", Q, False)):
            pts = _scan_pts(5, {2: TIE[cnt % 12]}, cnt)
            pl = _poly(kind, pts, 2, (0,), False, cnt, center=c + np.array([0.0, dy]), length=limit, kept=kept)
            out.append(_case(f"{KINDS[kind]}-cull-{what}", [pl], cnt, tags=("cull",)))
            cnt += 1
    return out


def _cross_cases():
    """Two polylines of one kind whose nearest points are equally near the row."""
    out, cnt = [], 300
    for kind in range(3):
        a = _poly(kind, _scan_pts(9, {4: TIE[(cnt + 1) % 12]}, cnt), 4, (0,), False, cnt, phi=0.4)
        b = _poly(kind, _scan_pts(65, {64: TIE[(cnt + 2) % 12]}, cnt + 1), 64, (0,), False, cnt, phi=0.9)
        out.append(_case(f"{KINDS[kind]}-cross", [a, b], cnt, tags=("cross",)))
        cnt += 1
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for kind in range(3):
        out += _scan_cases(kind)
    out += _straight_cases() + _cull_cases() + _cross_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# what a row of ``multi_crowd`` takes its polylines from: (points, slots that hold a tie point -- the first is expected)
MULTI_SPECS = ((9, (7, 8)), (65, (63, 64)), (129, (128,)), (64, (63,)), (200, (5, 130)), (7, (0,)), (127, (71, 72)), (8, (0, 7)), (2, (1,)))


def _multi_case(r, per_kind):
    """Row r of a multi-polyline crowd: per_kind[k] kept polylines of kind k, their expected points in three neighbouring directions
    (16 and 37 degrees apart), so that ONE pedestrian velocity leaves every static term above QUALIFY_TERM; the vehicles' velocities
    are chosen per polyline."""
    polys, m0 = [], 1 + 2 * (r % 6)
    for kind, count in enumerate(per_kind):
        for j in range(count):
            n_pts, slots = MULTI_SPECS[(r + j + 3 * kind) % len(MULTI_SPECS)]
            first = TIE[(m0 + j % 3) % 12]
            placed = {slots[0]: first}
            if len(slots) > 1:
                placed[slots[1]] = TIE[(m0 + j % 3 + 6) % 12]                     # the point opposite: same distance, opposite term
            pts = _scan_pts(n_pts, placed, r + j)
            alt = slots[1:] if len(slots) > 1 else ((int(np.argmin(np.where(np.arange(n_pts) == slots[0], np.inf, np.sum(pts * pts, axis=1)))),)
                                                    if n_pts > 1 else ())
            pl = _poly(kind, pts, slots[0], alt, len(slots) > 1, r + j)
            if kind:
                pl.dv = _dv_for(first, (0.6, -0.6)[r & 1], Dn=1.5)
            polys.append(pl)
    statics = [p for p in polys if p.kind == 1]
    ped_vel = _dv_for(TIE[(m0 + 1) % 12], (0.7, -0.7)[r & 1], Dn=1.5) if statics else None
    return _case(f"multi-{r}", polys, r, ped_vel=ped_vel, tags=("multi",))


# ---- crowds -------------------------------------------------------------------------------------------------------------------------
@dataclass
class Crowd:
    n: int
    loc: np.ndarray
    vel: np.ndarray
    waypoint: np.ndarray
    target_speed: np.ndarray
    radius: np.ndarray
    cases: list                                                 # per row
    poly: list = field(default_factory=lambda: [[], [], []])    # per kind: the Poly of every index k
    owner: list = field(default_factory=lambda: [[], [], []])   # per kind: the row that owns index k
    borders: list = field(default_factory=list)
    border_centers: np.ndarray = None
    border_lengths: np.ndarray = None
    static_obstacles: list = field(default_factory=list)
    dynamic_obstacles: list = field(default_factory=list)
    dynamic_vel: np.ndarray = None

    def geometry(self):
        return O.Geometry(self.borders, self.border_centers, self.border_lengths, self.static_obstacles, self.dynamic_obstacles,
                          self.dynamic_vel)

    def scene(self):
        """The crowd as a scene dict of ``SfmBatch.upload``."""
        return {"loc": self.loc, "vel": self.vel, "waypoint": self.waypoint, "target_speed": self.target_speed, "radius": self.radius,
                "borders": self.borders, "border_centers": self.border_centers, "border_lengths": self.border_lengths,
                "static_obstacles": self.static_obstacles, "dynamic_obstacles": self.dynamic_obstacles, "dynamic_vel": self.dynamic_vel}

    def points(self, kind, k):
        """Absolute points of polyline k of a kind."""
        return (self.borders[k] if kind == 0 else (self.static_obstacles, self.dynamic_obstacles)[kind - 1][k][1])

    def center(self, kind, k):
        return self.border_centers[k] if kind == 0 else (self.static_obstacles, self.dynamic_obstacles)[kind - 1][k][0]


def _fma_d2(ax, ay):
    """fmaf(ax, ax, ay * ay) of fp32 arrays: ay * ay rounded to fp32, ax * ax exact in float64, one rounding of the sum."""
    yy = (ay * ay).astype(np.float64)
    return (ax.astype(np.float64) * ax.astype(np.float64) + yy).astype(np.float32)


def assert_exact(c):
    """Every squared distance a case decides on -- pedestrian to each point and to the centre of each polyline of its own -- is the
    same number in fp32 (as the kernels form it: fp32 differences, fmaf(ax, ax, ay * ay), and the unfused form) and in float64, and
    below 2^13; every input is fp32-representable.  Returns the number of distances checked."""
    for a in (c.loc, c.vel, c.waypoint, c.radius, c.target_speed):
        assert np.array_equal(a, np.float32(a).astype(np.float64))
    checked = 0
    for kind in range(3):
        for k, row in enumerate(c.owner[kind]):
            x = c.loc[row, :2]
            pts = np.vstack([c.points(kind, k), np.asarray(c.center(kind, k))[None, :]])
            assert np.array_equal(pts, np.float32(pts).astype(np.float64)), (kind, k)
            d64 = pts - x
            d2_64 = d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]
            ax, ay = np.float32(x[0]) - np.float32(pts[:, 0]), np.float32(x[1]) - np.float32(pts[:, 1])
            assert np.array_equal(ax.astype(np.float64), -d64[:, 0]) and np.array_equal(ay.astype(np.float64), -d64[:, 1]), (kind, k)
            plain = (ax * ax + ay * ay).astype(np.float32)
            for d2_32 in (_fma_d2(ax, ay), _fma_d2(ay, ax), plain):
                assert d2_32.dtype == np.float32 and np.array_equal(d2_32.astype(np.float64), d2_64), (c.cases[row].name, kind, k)
            assert (d2_64 < D2_LIMIT).all(), (c.cases[row].name, kind, k, d2_64.max())
            assert np.array_equal(d2_64 * 256.0, np.round(d2_64 * 256.0)), (kind, k)           # 8 fraction bits
            checked += len(pts)
    return checked


def _assemble(row_cases, order, seed, z3):
    n = len(row_cases)
    rng = np.random.default_rng(seed)
    rows = np.arange(n)
    site = np.stack([(rows % SITE_W) * SITE, (rows // SITE_W) * SITE], axis=1)
    loc = np.zeros((n, 3))
    loc[:, :2] = site + PED_OFF[rows % 4]
    vel = np.zeros((n, 3))
    vel[:, :2] = np.array([c.ped_vel for c in row_cases]).reshape(n, 2)
    if z3:
        loc[:, 2] = 0.25 * (rows % 5)
        vel[:, 2] = 0.125 * ((rows % 3) - 1)
    wp = loc.copy()
    wp[:, :2] += np.array([4.0, -3.0])
    wp[:, 2] = 0.0
    c = Crowd(n, loc, vel, wp, np.full(n, TARGET_SPEED), np.full(n, RADIUS), list(row_cases))
    for kind in range(3):
        mine = [(r, pl) for r, case in enumerate(row_cases) for pl in case.polys if pl.kind == kind]
        if order == "random":
            mine = [mine[q] for q in rng.permutation(len(mine))]
        c.owner[kind] = np.array([r for r, _ in mine], dtype=np.int64)
        c.poly[kind] = [pl for _, pl in mine]
        pts = [loc[r, :2] + pl.pts for r, pl in mine]
        ctr = [loc[r, :2] + pl.center for r, pl in mine]
        if kind == 0:
            c.borders = pts
            c.border_centers = np.array(ctr).reshape(-1, 2)
            c.border_lengths = np.array([pl.length for _, pl in mine], dtype=np.float64)
        elif kind == 1:
            c.static_obstacles = list(zip(ctr, pts))
        else:
            c.dynamic_obstacles = list(zip(ctr, pts))
            c.dynamic_vel = np.array([pl.obs_vel for _, pl in mine]).reshape(-1, 2)
    assert_exact(c)
    return c


@functools.lru_cache(maxsize=None)
def crowd(n, order="rows", seed=0, start=0, z3=False):
    """Cases start, start + 1, ... (cyclically over ``cases()``) on n rows, row r on site r.  order "rows": case start + r on row r,
    polylines indexed in row order; "random": which case lands on which row, and which polyline on which index k, permuted from ``seed``."""
    all_cases = cases()
    idx = (start + np.arange(n)) % len(all_cases)
    if order == "random":
        idx = idx[np.random.default_rng(seed + 1000).permutation(n)]
    else:
        assert order == "rows", order
    return _assemble([all_cases[q] for q in idx], order, seed, z3)


@functools.lru_cache(maxsize=None)
def multi_crowd(n, per_kind=(3, 3, 3), order="rows", seed=0, z3=False):
    """Every row keeps per_kind[k] polylines of kind k (sum(per_kind) * n in all): more than the geometry finder's lists hold."""
    return _assemble([_multi_case(r, per_kind) for r in range(n)], order, seed, z3)


# ---- reference and expectations -------------------------------------------------------------------------------------------------------
GEO_FORCES = ("pedestrian_force",) + FORCE_OF_KIND


def config(use_ped_radius=False, max_speed_factor=None):
    """Stock parameters, the three geometry forces and the pedestrian force at A = 0 (the symmetric and the fused paths need the
    pedestrian force switched on; at A = 0 its terms are exactly 0 and a row's total is its geometry forces)."""
    from carla_social_force_model_amd.config import default_sfm_config
    cfg = default_sfm_config(GEO_FORCES)
    cfg["pedestrian_force"]["A"] = 0.0
    cfg["use_ped_radius"] = bool(use_ped_radius)
    if max_speed_factor is not None:
        cfg["max_speed_factor"] = max_speed_factor
    return cfg


@dataclass
class Ref:
    per: dict
    total: np.ndarray
    diag: dict


def reference(c, cfg):
    """Per-force results of ``O.tick_forces`` with NO tie allowance (tie_rel = 0): name -> (n, 3), total, diag name -> (exposure, absum)."""
    prm = O.OracleParams.from_config(cfg)
    diag = {}
    with np.errstate(all="ignore"):
        per, total, _ = O.tick_forces(c.loc, c.vel, c.waypoint, c.target_speed, c.radius, np.zeros(c.n, bool), c.geometry(), prm,
                                      theta_tol=P.THETA_TOL, tie_rel=0.0, diag=diag)
    return Ref(per, total, diag)


def expected_points(c):
    """From the designed slots alone: (point (n, 3, 2) -- absolute coordinates of the nearest point over the row's own polylines of each
    kind, NaN where it has none; item (n, 3) -- the index k of the polyline that holds it, -1 without; d2 (n, 3) exact).  Among
    polylines whose expected points are equally near, the lower index wins (np.argmin over the kind's points in CSR order)."""
    pt = np.full((c.n, 3, 2), np.nan)
    item = np.full((c.n, 3), -1, dtype=np.int64)
    d2 = np.full((c.n, 3), np.inf)
    for kind in range(3):
        for k, (row, pl) in enumerate(zip(c.owner[kind], c.poly[kind])):
            off = pl.pts[pl.exp]
            d = float(off[0] * off[0] + off[1] * off[1])
            if d < d2[row, kind]:
                d2[row, kind], item[row, kind] = d, k
                pt[row, kind] = c.loc[row, :2] + off
    return pt, item, d2


def kept(c):
    """(n, 3) bool: does the row keep a polyline of the kind (by design)?"""
    out = np.zeros((c.n, 3), bool)
    for kind in range(3):
        for row, pl in zip(c.owner[kind], c.poly[kind]):
            out[row, kind] |= pl.kept
    return out


def poly_term(c, kind, k, slot, prm):
    """The oracle's term of polyline k on its owner with the point at ``slot`` taken for the nearest (forces.py:158-165 /
    :233-270 through ``O.unit_and_norm`` and ``O.moussaid_term``).  Returns (force (2,), exposure)."""
    row, pl = c.owner[kind][k], c.poly[kind][k]
    x, p = c.loc[row, :2], c.loc[row, :2] + pl.pts[slot]
    if kind == 0:
        dirn, dist = O.unit_and_norm((x - p)[None, :])
        if prm.use_ped_radius:
            dist = dist - c.radius[row]
        return (dirn * (prm.border_a * np.exp(-dist / prm.border_b))[:, None])[0], 0.0
    e, dist = O.unit_and_norm((p - x)[None, :])
    if prm.use_ped_radius:
        dist = dist - c.radius[row]
    ov = pl.obs_vel if kind == 2 else np.zeros(2)
    with np.errstate(all="ignore"):
        F, ex, _ = O.moussaid_term(e, dist, (c.vel[row, :2] - ov)[None, :], prm.static if kind == 1 else prm.dynamic, P.THETA_TOL)
    return F[0], float(ex[0])


def is_straight(pts):
    """sfm_set_borders' test (sfm_capi.hip) restated: P >= 8 and every point within 2 % of the spacing of a + (b - a) j / (P - 1)."""
    n_pts = len(pts)
    if n_pts < 8:
        return False
    a, ab = pts[0], pts[-1] - pts[0]
    spacing = float(np.hypot(*ab)) / (n_pts - 1)
    if not spacing > 1e-6:
        return False
    ideal = a[None, :] + np.arange(n_pts)[:, None] * ab[None, :] / (n_pts - 1)
    return bool((np.hypot(*(pts - ideal).T) <= 0.02 * spacing).all())


# ---- the geometry finder's deal (sfm_kernels.hip geo_find), restated for the host-side count of the overflow test ------------------------
GEO_WAVES, GEO_ITEMS = 16, 32


def finder_positions(c, n_slices=1):
    """Per kind, for every polyline index k: (tile, wave of the tile's n_slices x 16, position in that wave's sequence of KEPT polylines)
    for the tile of its owner -- positions >= GEO_ITEMS are scanned on the spot by the finder's second pass.  Restates geo_find's deal:
    polylines go to wave (dealt + k) mod n_gwaves in runs of 1 << run_log, borders first, each kind carrying on where the last ended;
    a wave meets its polylines trip by trip, lane by lane.  A polyline counts for a tile when a row of the tile keeps it."""
    n_g = GEO_WAVES * n_slices
    keep_tile = []                                          # per kind: (K, tiles) bool
    n_t = (c.n + 63) // 64
    for kind in range(3):
        m = np.zeros((len(c.owner[kind]), n_t), bool)
        for k, (row, pl) in enumerate(zip(c.owner[kind], c.poly[kind])):
            m[k, row // 64] = pl.kept
        keep_tile.append(m)
    out = [np.full((len(c.owner[kind]), 3), -1, dtype=np.int64) for kind in range(3)]
    for t in range(n_t):
        for gw in range(n_g):
            pos, dealt = 0, 0
            for kind in range(3):
                K = len(c.owner[kind])
                g = (gw + n_g - dealt % n_g) % n_g
                dealt += K
                run_log = 3 if K >= 64 * n_g else 2 if K >= 32 * n_g else 1 if K >= 16 * n_g else 0
                for base in range(0, K, 64 * n_g):
                    for lane in range(64):
                        k = base + ((((lane >> run_log) * n_g + g) << run_log) | (lane & ((1 << run_log) - 1)))
                        if k < K and keep_tile[kind][k, t]:
                            if c.owner[kind][k] // 64 == t:
                                out[kind][k] = (t, gw, pos)
                            pos += 1
    return out


# ---- the crowds both test files use ---------------------------------------------------------------------------------------------------
BATCH_SIZES = (3, 64, 65, 128, 130, 300)       # the batch kernel's 4 / 2 / 1 j-slice forms, one and two passes
OBSERVE_SIZES = (40, 65, 300)                  # the role-split form (N <= 64) and the one-wave-per-64 form
MULTI_KINDS = ((3, 3, 3), (9, 0, 0), (0, 9, 0))


def covering_crowds(n, z3=False):
    """Crowds of n rows, cases and polyline indices permuted, that together hold every case."""
    total = len(cases())
    if n >= total:
        return [crowd(n, "random", 7, 0, z3)]
    return [crowd(n, "random", 10 + s, n * s, z3) for s in range((total + n - 1) // n)]


def scene_crowds(sizes, z3=False, seed=20):
    out, start = [], 0
    for q, n in enumerate(sizes):
        out.append(crowd(n, "random", seed + q, start % len(cases()), z3))
        start += n
    return out


def covered(crowds):
    return {c.name for cr in crowds for c in cr.cases} == {c.name for c in cases()}
