"""DESIGNED ROWS for the per-pedestrian tick update (tests/test_update_cases_host.py on the CPU, tests/test_update_cases_gpu.py on the
GPU).  NumPy only, no GPU code here.

The update every tick runs -- acceleration towards the waypoint, v' = cap(v + dt F), x' = x + dt v', the arrival test on the pre-move
position, the next waypoint from the counter stream -- is a chain of DECISIONS: strict ``<`` on the planar distance
(pedestrian_simulation.py:95), ``min(1, cap / speed)`` (stateutils.py:18-23), the zero-vector guards (stateutils.py:85-92).  The other
tests exempt the rows near a decision; here every row sits ON one, and nothing is exempted.

A CASE is one pedestrian alone on its own site of a lattice of pitch ``PITCH``, wide enough that the pedestrian force between sites is
exactly 0 in fp32 (the host test asserts it from the oracle).  EXACTNESS: every coordinate is a multiple of Q = 2^-8 m below 2^14 m,
every velocity and target speed a dyadic number of a few bits, so w - x, fmaf(ax, ax, ay * ay) of a designed offset and the designed
v + dt F are exact in fp32: the device's comparison IS the exact comparison.

PARAMETER SETS (both tau 0.5, max_speed_factor 2.0, powers of two so that the ties can be hit):
  "tie"   dt = tau = 0.5:  v + dt F = ts e exactly where e is exact -- on the waypoint (e = 0) that is the ZERO VECTOR for any v.
  "half"  dt = 0.25:       v + dt F = (v + ts e) / 2 -- on the waypoint v / 2, which puts the speed where the case wants it.
A case names the sets it is designed for, the arrival threshold it needs (2.0 stock, 2.5 for the Pythagorean offsets, None: either),
and states its outcome: ``arrived``, ``capped`` and, per set, the v' that the IEEE forms must return bit for bit (``v_exact``).

``crowd(n, pset, thr, z3, shuffle)`` repeats the cases that fit over n rows, row r on site r (``shuffle``: on site perm[r], so that a
spatial re-sort of the rows is not the identity).  ``expectation`` is the oracle's free_step with the acceleration force alone.
"""
import functools
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from oracle import sfm_oracle as O

Q = 2.0 ** -8
PITCH = 512.0
SITE_W = 32                    # sites per lattice row: N = 1024 fills 32 x 32, every |coordinate| < 2^14
COORD_LIMIT = 2.0 ** 14
TAU = 0.5
MSF = 2.0
PSETS = {"tie": 0.5, "half": 0.25}      # name -> dt
THRESHOLDS = (2.0, 2.5)
SEED, WORLD_SIDE = 20260, 1.0           # every drawn waypoint lies in [0, 1)^2: site 0 (the origin) is inside the stream's own square
RADIUS = 0.25
PED_OFF = np.array([(0.0, 0.0), (3 * Q, -2 * Q), (-5 * Q, 1.0), (2.0, 7 * Q)])      # where on its site a pedestrian stands
KINDS = ("at", "inside", "outside", "on", "pre-out-post-in", "pre-in-post-out", "cap-tie", "cap-twice", "cap-above", "cap-below",
         "ts0-moving", "zero-sum", "rest")
KINDS_3D = ("dz-inside", "dz-outside", "cap-3d", "cap-3d-tie", "acc-z")


@dataclass
class Case:
    name: str
    kind: str
    off: tuple                          # waypoint - x, planar
    v: tuple                            # (vx, vy, vz)
    ts: float
    arrived: bool
    psets: tuple = ("tie", "half")
    thr: float = None                   # the threshold the outcome is stated for; None: both
    z: float = 0.0
    capped: dict = field(default_factory=dict)        # pset -> bool (unstated: not capped)
    v_exact: dict = field(default_factory=dict)       # pset -> (3,) v' the IEEE forms return bit for bit
    zero: tuple = ()                                  # psets in which v' = 0 exactly and x' = x ON EVERY PATH
    what: str = ""                                    # the outcome in words

    @property
    def z3(self):
        return self.z != 0.0 or self.v[2] != 0.0


def _both(v):
    return {"tie": v, "half": v}


def _cases():
    V = (0.5, -0.25, 0.0)
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    # ---- arrival: strict <, planar, pre-move --------------------------------------------------------------------------------------------
    for tag, off in (("x", (2.0, 0.0)), ("y", (0.0, -2.0))):
        add(f"at-{tag}", "at", off, V, 1.25, False, thr=2.0, what="d = thr exactly: not arrived (strict <)")
    for tag, off in (("a", (1.5, 2.0)), ("b", (-2.0, 1.5))):
        add(f"at-pyth-{tag}", "at", off, V, 1.25, False, thr=2.5, what="d^2 = 2.25 + 4 = 2.5^2 exactly: not arrived")
    add("inside-x", "inside", (2.0 - Q, 0.0), V, 1.25, True, thr=2.0, what="one quantum inside: arrived")
    add("inside-y", "inside", (0.0, -2.0 + Q), V, 1.25, True, thr=2.0, what="one quantum inside: arrived")
    add("inside-pyth", "inside", (1.5, 2.0 - Q), V, 1.25, True, thr=2.5, what="one quantum inside: arrived")
    add("inside-pyth-b", "inside", (-2.0 + Q, 1.5), V, 1.25, True, thr=2.5, what="one quantum inside: arrived")
    add("outside-x", "outside", (2.0 + Q, 0.0), V, 1.25, False, thr=2.0, what="one quantum outside: not arrived")
    add("outside-y", "outside", (0.0, -2.0 - Q), V, 1.25, False, thr=2.0, what="one quantum outside: not arrived")
    add("outside-pyth", "outside", (1.5 + Q, 2.0), V, 1.25, False, thr=2.5, what="one quantum outside: not arrived")
    add("outside-pyth-b", "outside", (-2.0, 1.5 + Q), V, 1.25, False, thr=2.5, what="one quantum outside: not arrived")
    # on the waypoint: the desired direction is the zero vector (stateutils.py:85-92).  tie: v + dt F = v - v = 0 (sp = 1 on the IEEE
    # forms, fac = 0 on the RSQ forms); half: v / 2, under the cap
    add("on-waypoint", "on", (0.0, 0.0), (0.5, -0.25, 0.0), 1.25, True, v_exact={"tie": (0.0, 0.0, 0.0), "half": (0.25, -0.125, 0.0)},
        zero=("tie",), what="on the waypoint: arrived, e = 0; tie: v' = 0, half: v' = v / 2")
    add("on-waypoint-slow", "on", (0.0, 0.0), (0.25, 0.125, 0.0), 0.5, True, v_exact={"tie": (0.0, 0.0, 0.0), "half": (0.125, 0.0625, 0.0)},
        zero=("tie",), what="as on-waypoint, at a quarter of a metre per tick at the most (the row of the stream-square test)")
    add("zero-sum", "zero-sum", (0.0, 0.0), (1.0, 0.75, 0.0), 1.25, True, psets=("tie",), v_exact={"tie": (0.0, 0.0, 0.0)}, zero=("tie",),
        what="v + dt F = 0 exactly: v' = 0, x' = x")
    # the decision follows the PRE-move position
    for thr in THRESHOLDS:
        add(f"pre-out-post-in-{thr}", "pre-out-post-in", (thr + 0.25, 0.0), (2.0, 0.0, 0.0), 1.25, False, thr=thr,
            what="a quarter of a metre outside before the move, inside after it: not arrived")
        add(f"pre-in-post-out-{thr}", "pre-in-post-out", (thr - 0.25, 0.0), (-4.0, 0.0, 0.0), 1.0, True, psets=("half",), thr=thr,
            what="a quarter of a metre inside before the move, v' = -1.5 carries it 0.125 m outside: arrived")
    add("overshoot", "pre-in-post-out", (0.5, 0.0), (0.0, 0.0, 0.0), 8.0, True, psets=("tie",), v_exact={"tie": (8.0, 0.0, 0.0)},
        what="inside before the move, v' = ts e = 8 carries it 3.5 m past the waypoint: arrived")
    # ---- cap (set half, on the waypoint: v + dt F = v / 2 exactly) --------------------------------------------------------------------
    add("cap-tie", "cap-tie", (0.0, 0.0), (1.5, 2.0, 0.0), 0.625, True, psets=("half",), v_exact={"half": (0.75, 1.0, 0.0)},
        what="|v + dt F| = 1.25 = ts * factor exactly: min(1, 1) = 1, returned bit for bit")
    add("cap-tie-b", "cap-tie", (0.0, 0.0), (-2.0, 1.5, 0.0), 0.625, True, psets=("half",), v_exact={"half": (-1.0, 0.75, 0.0)},
        what="|v + dt F| = 1.25 = ts * factor exactly")
    add("cap-twice", "cap-twice", (0.0, 0.0), (1.5, 2.0, 0.0), 0.3125, True, psets=("half",), capped={"half": True},
        v_exact={"half": (0.375, 0.5, 0.0)}, what="|v + dt F| = 1.25 = twice the cap: scaled by exactly 0.5")
    add("cap-above", "cap-above", (0.0, 0.0), (1.5, 2.0 + 2 * Q, 0.0), 0.625, True, psets=("half",), capped={"half": True},
        what="one quantum above the cap: capped")
    add("cap-below", "cap-below", (0.0, 0.0), (1.5, 2.0 - 2 * Q, 0.0), 0.625, True, psets=("half",),
        v_exact={"half": (0.75, 1.0 - Q, 0.0)}, what="one quantum below the cap: v + dt F bit for bit")
    add("ts0-moving", "ts0-moving", (3.0, 0.0), (1.0, -0.5, 0.0), 0.0, False, capped={"half": True},
        v_exact=_both((0.0, 0.0, 0.0)), zero=("tie", "half"), what="target speed 0: v' = 0 exactly, x' = x (tie: v + dt F = 0; half: cap 0)")
    add("ts0-moving-on", "ts0-moving", (0.0, 0.0), (-0.75, 1.0, 0.0), 0.0, True, capped={"half": True},
        v_exact=_both((0.0, 0.0, 0.0)), zero=("tie", "half"), what="target speed 0 on the waypoint: v' = 0 exactly, x' = x")
    add("ts0-creeping", "ts0-moving", (3.0, 0.0), (2.0 ** -79, 0.0, 0.0), 0.0, False, capped={"half": True},
        v_exact=_both((0.0, 0.0, 0.0)), zero=("tie", "half"),
        what="target speed 0 at 2^-79 m/s: half: |v + dt F|^2 = 2^-160 underflows to 0 in fp32, and v' is still 0 exactly, not 2^-80")
    add("rest", "rest", (0.0, 0.0), (0.0, 0.0, 0.0), 0.0, True, v_exact=_both((0.0, 0.0, 0.0)), zero=("tie", "half"),
        what="at rest on the waypoint with target speed 0: stays put")
    # ---- 3-D ---------------------------------------------------------------------------------------------------------------------------
    add("dz-inside", "dz-inside", (1.0, 0.5), (0.5, -0.25, 0.125), 1.25, True, z=10.0, what="|dz| = 10 m, planar offset inside: arrived")
    add("dz-at", "dz-inside", (2.0 - Q, 0.0), (0.5, -0.25, -0.125), 1.25, True, thr=2.0, z=10.0, what="|dz| = 10 m, one quantum inside: arrived")
    add("dz-outside", "dz-outside", (3.0, 0.0), (0.5, -0.25, 0.125), 1.25, False, z=0.0, what="z equals the waypoint's, planar offset outside: not arrived")
    add("dz-outside-at", "dz-outside", (2.0, 0.0), (0.5, -0.25, 0.125), 1.25, False, thr=2.0, z=0.0, what="z equals the waypoint's, d = thr: not arrived")
    add("cap-3d", "cap-3d", (0.0, 0.0), (1.5, 1.0, 2.0), 0.625, True, psets=("half",), z=1.0, capped={"half": True},
        what="planar speed 0.90 below the cap 1.25, 3-D speed 1.35 above: capped, all three components scaled")
    add("cap-3d-tie", "cap-3d-tie", (0.0, 0.0), (1.0, 2.0, 2.0), 0.75, True, psets=("half",), z=1.0, v_exact={"half": (0.5, 1.0, 1.0)},
        what="3-D speed 1.5 = cap exactly: bit for bit")
    add("acc-z", "acc-z", (0.0, 0.0), (0.5, 0.25, 0.5), 1.25, True, z=2.0, v_exact={"tie": (0.0, 0.0, 0.0), "half": (0.25, 0.125, 0.25)},
        zero=("tie",), what="acceleration z = -v_z / tau: tie: v'_z = 0, half: v'_z = v_z / 2")
    add("acc-z-off", "acc-z", (4.0, 0.0), (0.5, 0.25, 0.5), 1.25, False, z=2.0,
        v_exact={"tie": (1.25, 0.0, 0.0), "half": (0.875, 0.125, 0.25)}, what="4 m from the waypoint (e = (1, 0) exactly): v'_z as above")
    assert len({c.name for c in out}) == len(out) and {c.kind for c in out} == set(KINDS + KINDS_3D)
    return tuple(out)


CASES = _cases()


def fitting(pset, thr, z3):
    return tuple(c for c in CASES if pset in c.psets and c.thr in (None, thr) and (z3 or not c.z3))


# ---- crowds ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class Crowd:
    n: int
    pset: str
    thr: float
    z3: bool
    loc: np.ndarray
    vel: np.ndarray
    waypoint: np.ndarray
    target_speed: np.ndarray
    radius: np.ndarray
    cases: list

    @property
    def dt(self):
        return PSETS[self.pset]

    def scene(self):
        """The crowd as a scene dict of ``SfmBatch.upload``."""
        return {"loc": self.loc, "vel": self.vel, "waypoint": self.waypoint, "target_speed": self.target_speed, "radius": self.radius}

    def mask(self, f):
        return np.array([bool(f(c)) for c in self.cases])

    @property
    def arrived(self):
        return self.mask(lambda c: c.arrived)

    @property
    def capped(self):
        return self.mask(lambda c: c.capped.get(self.pset, False))

    @property
    def zero(self):
        return self.mask(lambda c: self.pset in c.zero)

    def v_exact(self):
        """(rows, (k, 3) values) of the rows whose v' the IEEE forms return bit for bit."""
        rows = np.flatnonzero(self.mask(lambda c: self.pset in c.v_exact))
        return rows, np.array([self.cases[r].v_exact[self.pset] for r in rows], dtype=np.float64).reshape(-1, 3)

    def kinds(self):
        out = {}
        for c in self.cases:
            out[c.kind] = out.get(c.kind, 0) + 1
        return out


def is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array_equal(a, a.astype(np.float32).astype(np.float64))


@functools.lru_cache(maxsize=None)
def crowd(n, pset, thr=2.0, z3=False, shuffle=False, start=0):
    fit = fitting(pset, thr, z3)
    return assemble([fit[(start + r) % len(fit)] for r in range(n)], pset, thr, z3, shuffle)


def assemble(row_cases, pset, thr=2.0, z3=False, shuffle=False):
    n = len(row_cases)
    rows = np.arange(n)
    site_of = np.random.default_rng(77).permutation(n) if shuffle else rows
    site = np.stack([(site_of % SITE_W) * PITCH, (site_of // SITE_W) * PITCH], axis=1)
    loc = np.zeros((n, 3))
    loc[:, :2] = site + PED_OFF[rows % 4]
    vel = np.array([c.v for c in row_cases], dtype=np.float64).reshape(n, 3)
    if z3:
        loc[:, 2] = [c.z for c in row_cases]
    else:
        assert not vel[:, 2].any()
    wp = np.zeros((n, 3))
    wp[:, :2] = loc[:, :2] + np.array([c.off for c in row_cases]).reshape(n, 2)
    c = Crowd(n, pset, thr, z3, loc, vel, wp, np.array([c.ts for c in row_cases]), np.full(n, RADIUS), row_cases)
    assert_exact(c)
    return c


def assert_exact(c):
    """Every input is an fp32 number on the quantum grid below 2^14; w - x is exact in fp32 and its squared length is the same number
    as fmaf(ax, ax, ay * ay), as the unfused form and in float64; thr^2 is exact."""
    for a in (c.loc, c.vel, c.waypoint, c.target_speed, c.radius, np.array([c.thr, c.dt, TAU, MSF, c.thr * c.thr])):
        assert is_f32(a)
    for a in (c.loc, c.waypoint):
        assert np.array_equal(a / Q, np.round(a / Q)) and (np.abs(a) < COORD_LIMIT).all()
    x32, w32 = np.float32(c.loc[:, :2]), np.float32(c.waypoint[:, :2])
    a32 = w32 - x32
    a64 = c.waypoint[:, :2] - c.loc[:, :2]
    assert a32.dtype == np.float32 and np.array_equal(a32.astype(np.float64), a64)
    d2_64 = a64[:, 0] * a64[:, 0] + a64[:, 1] * a64[:, 1]
    yy = (a32[:, 1] * a32[:, 1]).astype(np.float64)
    fma = (a32[:, 0].astype(np.float64) * a32[:, 0].astype(np.float64) + yy).astype(np.float32)
    plain = (a32[:, 0] * a32[:, 0] + a32[:, 1] * a32[:, 1]).astype(np.float32)
    for d2 in (fma, plain):
        assert d2.dtype == np.float32 and np.array_equal(d2.astype(np.float64), d2_64)
    assert np.array_equal(d2_64 * 65536.0, np.round(d2_64 * 65536.0))


# ---- configuration and reference --------------------------------------------------------------------------------------------------------
def config(pset, ped="off", rad=False, border=False):
    """tau 0.5, max_speed_factor 2.0; the acceleration force, and the pedestrian force: "off", "A0" (switched on with A = 0: its terms
    are exactly 0, and the paths that only run with the force on -- the symmetric pair kernel, the fused tick -- are reached) or
    "stock" (the stock parameters: exactly 0 between sites by the lattice pitch)."""
    from carla_social_force_model_amd.config import default_sfm_config
    assert pset in PSETS and ped in ("off", "A0", "stock")
    cfg = default_sfm_config(("acceleration_force",) if ped == "off" else ("acceleration_force", "pedestrian_force"))
    if ped == "A0":
        cfg["pedestrian_force"]["A"] = 0.0
    cfg["goal_force"] = {"tau": TAU}
    cfg["max_speed_factor"] = MSF
    cfg["use_ped_radius"] = bool(rad)
    if border:                                                     # (the stock border parameters; the cells' one border is 10 km away)
        cfg["forces"]["border_force"] = True
    return cfg


def acc_params(pset):
    return O.OracleParams.from_config(config(pset, "off"))


@dataclass
class Expect:
    v: np.ndarray              # (n, 3) float64: O.new_velocities of the acceleration force
    arrived: np.ndarray        # (n,) bool: O.arrived
    waypoint: np.ndarray       # (n, 2) after a redrawing tick: bitwise the fp32 draw on arrived rows, the old waypoint elsewhere
    draws: np.ndarray          # (n,) after a redrawing tick from ``d0``


def expectation(c, d0=None, key=None, seed=SEED, side=WORLD_SIDE):
    """The oracle's free_step on the crowd with the acceleration force alone (the pedestrian force is exactly 0 by isolation)."""
    prm = acc_params(c.pset)
    d0 = np.zeros(c.n, dtype=np.int64) if d0 is None else np.asarray(d0, dtype=np.int64)
    _, v_new, wp, draws = O.free_step(c.loc, c.vel, c.waypoint, c.target_speed, c.radius, np.zeros(c.n, bool), d0, O.Geometry(), prm, c.dt,
                                      c.thr, seed, side)
    hit = O.arrived(c.loc, c.waypoint, c.thr)
    if key is not None:                                           # rows keyed by something else than their position in the crowd
        wp = c.waypoint.copy()
        wp[hit, :2] = O.redraw_waypoint(np.asarray(key)[hit], draws[hit], seed, side)
    return Expect(v_new, hit, wp[:, :2], draws)


# ---- exact arithmetic ---------------------------------------------------------------------------------------------------------------
def round_f32(fr):
    """A rational number rounded ONCE to fp32 (nearest, ties to even; subnormals included; no overflow expected)."""
    fr = Fraction(fr)
    if fr == 0:
        return 0.0
    sign, a = (-1.0, -fr) if fr < 0 else (1.0, fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    k, rem = divmod(a, ulp)
    k = int(k)
    if rem * 2 > ulp or (rem * 2 == ulp and k % 2 == 1):
        k += 1
    return sign * float(k * ulp)


def fma_f32(dt, v, x):
    """Component by component the correctly rounded fp32 fma(dt, v, x) of fp32 inputs, formed in rational arithmetic (a float64
    product-sum rounds twice)."""
    v, x = np.asarray(v, dtype=np.float64), np.asarray(x, dtype=np.float64)
    assert is_f32(v) and is_f32(x) and is_f32(dt) and v.shape == x.shape
    out = np.empty(v.shape)
    fdt = Fraction(float(dt))
    for idx in np.ndindex(*v.shape):
        out[idx] = round_f32(fdt * Fraction(float(v[idx])) + Fraction(float(x[idx])))
    return out


def ulp_distance(a, b):
    """Worst distance in fp32 units in the last place between two arrays of fp32 values (measured in the ulp of the larger)."""
    a32, b32 = np.float32(a), np.float32(b)
    scale = np.spacing(np.maximum(np.abs(a32), np.abs(b32)).astype(np.float32)).astype(np.float64)
    d = np.abs(a32.astype(np.float64) - b32.astype(np.float64)) / scale
    return float(np.max(d)) if d.size else 0.0


def ieee_update_f32(c):
    """The IEEE form of the update restated in NumPy float32, operation by operation as sfm_interaction.h writes it except that a
    product-sum is two roundings here (NumPy has no fma): (v', x') float32."""
    f = np.float32
    x, w, v, ts = f(c.loc), f(c.waypoint[:, :2]), f(c.vel), f(c.target_speed)
    inv_tau, dt, msf = f(1.0) / f(TAU), f(c.dt), f(MSF)
    t = w - x[:, :2]
    nrm = np.sqrt(t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1])
    inv = np.where(nrm == 0, f(1.0), f(1.0) / np.where(nrm == 0, f(1.0), nrm)).astype(f)
    F = np.zeros_like(v)
    F[:, 0] = (ts * (t[:, 0] * inv) - v[:, 0]) * inv_tau
    F[:, 1] = (ts * (t[:, 1] * inv) - v[:, 1]) * inv_tau
    F[:, 2] = (f(0.0) - v[:, 2]) * inv_tau
    nv = dt * F + v
    sp = np.sqrt(nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1] + nv[:, 2] * nv[:, 2])
    sp = np.where(sp == 0, f(1.0), sp).astype(f)
    fac = np.minimum(f(1.0), (ts * msf) / sp).astype(f)
    nv = (nv * fac[:, None]).astype(f)
    assert nv.dtype == np.float32
    return nv, (dt * nv + x).astype(f)


# ---- the crowds both test files use ---------------------------------------------------------------------------------------------------
ENGINE_CROWDS = [(65, False), (257, False), (65, True), (257, True), (320, False), (320, True), (128, False), (256, True), (1024, False)]
BATCH_SIZES = (1, 2, 63, 65, 300)


def engine_crowds():
    """Every (n, pset, thr, z3) the handle's cells run."""
    return [crowd(n, pset, thr, z3) for n, z3 in ENGINE_CROWDS for pset in PSETS for thr in THRESHOLDS] + \
           [crowd(320, pset, 2.0, False, True) for pset in PSETS]


def batch_crowds(z3):
    """Scenes of 1, 2, 63, 65 and 300 rows, once per (parameter set, threshold): twenty scenes, neighbours on different sets."""
    out, start = [], 0
    for pset, thr in (("tie", 2.0), ("half", 2.5), ("half", 2.0), ("tie", 2.5)):
        for n in BATCH_SIZES:
            out.append(crowd(n, pset, thr, z3, False, start % len(fitting(pset, thr, z3))))
            start += n
    return out


FAR_BORDER = (np.array([[-10240.0, -10240.0], [-10239.0, -10240.0]]), np.array([-10239.5, -10240.0]), 1.0)      # points, centre, length


def start_of(name, pset, thr=2.0, z3=False):
    """The ``start`` that puts the named case on row 0 (site 0, the origin)."""
    return [c.name for c in fitting(pset, thr, z3)].index(name)


def kinds_needed(pset, thr, z3):
    return {c.kind for c in fitting(pset, thr, z3)}
