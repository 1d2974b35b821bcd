"""Scenarios, oracle references and the two conditions of the parameter-space tests (tests/test_param_space_host.py on the CPU,
tests/test_param_space_gpu.py on the GPU).  No GPU code here: everything below is the oracle's side of a cell.

Conditions every cell must meet ON THE ORACLE ALONE, asserted by ``conditions``:
  * at most 10 % of the cell's rows carry a non-zero discontinuity exposure (they stay checked; they only receive the reference's
    own jump as allowance);
  * the mean conditioning weight of every row's terms, ``_parity.diagnostics``' max_amp = max_i (A_i / sum_j |f_ij| - 1), stays
    <= 1.0 -- the ceiling tests/test_hip_parity.py's FULL_SIZE_CEILINGS uses -- so that the conditioned scale cannot do the work of
    the test."""
import numpy as np

import _param_sets as psets
import _parity as P
from carla_social_force_model_amd import scenarios
from oracle import c_oracle
from oracle import sfm_oracle as O

MAX_EXPOSED_SHARE = 0.10
MAX_AMP = 1.0
READBACK_MSF = 1e7
PED_ACC = ("acceleration_force", "pedestrian_force")
ALL5 = scenarios.ALL_FORCES
VEHICLE_SPEED = 0.25          # of make_scenario's 0 .. 14 m/s: at 14 m/s next to a pedestrian B = gamma |lambda dv + e| is ~10 and one
                              # dynamic-obstacle term's conditioning weight alone passes MAX_AMP (the existing dynamic-obstacle tests
                              # use check_velocity_conditioned for that reason); these tests keep the plain bounds


def scene(n, seed, z_spread=0.0, geo=True, density=0.25):
    """A generic crowd (jittered grid, velocities towards random waypoints with noise: no pair is at rest) with, if ``geo``,
    ~n/50 borders (most exposed rows are argmin ties on their 0.1 m samples), ~n/80 static obstacles and ~n/200 slowed vehicles."""
    nb, ns, nd = (max(3, n // 50), max(2, n // 80), max(1, n // 200)) if geo else (0, 0, 0)
    sc = scenarios.make_scenario(n, seed, n_borders=min(nb, 40), n_static=min(ns, 20), n_dynamic=min(nd, 6), z_spread=z_spread,
                                 density=density, border_len=(3.0, 15.0))
    if nd:
        sc.dynamic_vel = scenarios._f32(sc.dynamic_vel * VEHICLE_SPEED)
    rng = np.random.default_rng(seed + 17)
    sc.radius = np.float32(rng.uniform(0.2, 0.45, n)).astype(np.float64)
    return sc


def geometry(sc):
    return O.Geometry(sc.borders, sc.border_centers, sc.border_lengths, sc.static_obstacles, sc.dynamic_obstacles, sc.dynamic_vel)


class Ref:
    """The oracle's side of one tick: per-force results with their exposure and scale (NumPy oracle, which models argmin ties
    and cull edges), v', and what the conditions need (C oracle: the unweighted sum of term magnitudes)."""

    def __init__(self, loc, vel, sc, cfg, dt, crossing=None, geom=None, rows=None):
        n = len(loc)
        self.prm = prm = O.OracleParams.from_config(cfg)
        self.dt = dt
        crossing = np.zeros(n, bool) if crossing is None else crossing
        geom = geometry(sc) if geom is None else geom
        i0, i1 = (0, n) if rows is None else rows
        self.rows = (i0, i1)
        plain = np.zeros(i1 - i0)
        with np.errstate(all="ignore"):
            if rows is None:
                self.diag = {}
                self.per, self.total, _ = O.tick_forces(loc, vel, sc.waypoint, sc.target_speed, sc.radius, crossing, geom, prm,
                                                        theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=self.diag)
                self.v_new = O.new_velocities(vel, self.total, sc.target_speed, dt, prm.max_speed_factor)
                _, _, _, _, absum = c_oracle.tick(loc, vel, sc.waypoint, sc.target_speed, sc.radius, crossing, geom, prm, dt,
                                                  theta_tol=P.THETA_TOL, plain=plain)
            else:        # a block of rows of a large crowd, C oracle alone: total only (no border / obstacle forces in those cells)
                assert not any(prm.enabled[k] for k in O.FORCE_NAMES[2:])
                self.per, self.total, self.v_new, expo, absum = c_oracle.tick(loc, vel, sc.waypoint, sc.target_speed, sc.radius,
                                                                              crossing, geom, prm, dt, rows=rows,
                                                                              theta_tol=P.THETA_TOL, plain=plain)
                self.diag = {"total": (expo, absum)}
        self.absum_c, self.plain = absum, plain
        ok = ~np.isnan(self.total).any(axis=1)
        self.max_amp = float(np.max(np.nan_to_num(absum[ok]) / np.maximum(plain[ok], 1e-300) - 1.0)) if ok.any() else 0.0
        self.exposed = int((np.nan_to_num(self.diag["total"][0]) > 0).sum())
        self.share = self.exposed / max(1, i1 - i0)

    def conditions(self, label, literal=True):
        """``literal`` False -- only for the cells whose size is fixed at N >= 4096 (the list cutoff and the fused tick at their full sizes): there the share of rows with a NON-ZERO
        exposure is a property of N, not of the parameters (every row has thousands of partners, each with a ~2e-5 chance of a
        theta within THETA_TOL of 0 or of the wrap, and a far partner's exposure of 1e-100 m/s^2 still counts: the STOCK c2 crowd
        has 9.3 % such rows, stock at N = 98 304 has 91 %).  Those cells cap the rows whose exposure exceeds ATOL instead, the
        floor check_force grants every row anyway: a smaller exposure cannot change a row's verdict by more than that floor."""
        expo = np.nan_to_num(self.diag["total"][0])
        n = self.rows[1] - self.rows[0]
        share = self.share if literal else material_share(self)
        assert share <= MAX_EXPOSED_SHARE, f"{label}: {share:.1%} of {n} rows exposed (> 10 %; literal share {self.share:.1%})"
        assert self.max_amp <= MAX_AMP, f"{label}: max_amp {self.max_amp:.3g} > {MAX_AMP}"
        return share, self.max_amp

    def check_forces(self, label, forces_of):
        """``forces_of(name) -> (n,3)``: every enabled force and the total, ``_parity.check_force``."""
        worst = 0.0
        for name in [k for k in O.FORCE_NAMES if k in self.per and k in self.diag] + ["total"]:
            ex, ab = self.diag[name]
            ref = self.total if name == "total" else self.per[name]
            got = forces_of(name)[self.rows[0]:self.rows[1]]
            worst = max(worst, P.check_force(f"{label}/{name}", got, ref, ab, ex)[0])
        return worst

    def check_velocity(self, v_dev):
        return P.check_velocity(v_dev[self.rows[0]:self.rows[1]], self.v_new, self.diag["total"][0], self.dt)


def material_share(ref):
    """Share of ``ref``'s rows whose exposure exceeds ATOL (``Ref.conditions`` with literal=False says when and why)."""
    expo = np.nan_to_num(ref.diag["total"][0])
    return float((expo > P.ATOL).sum()) / max(1, ref.rows[1] - ref.rows[0])


# ---- the list cutoff must have something to lose --------------------------------------------------------------------------------
def stock_reach_dropped_power(sc, cfg, stock_cfg, rows):
    """Per row i in ``rows``: the float64 sum of |f_ij| over the partners j whose TILE PAIR (tiles of 64 consecutive rows, the
    crowd in the order given) a reach built from ``stock_cfg``'s pedestrian gamma / lambda would drop --
    box distance > gamma_stock 41 ln2 (1 + lambda_stock (vmax_a + vmax_b)) [+ 2 r_max with use_ped_radius], the rule of DESIGN.md
    section 3.5 -- evaluated with ``cfg``'s own parameters; and that row's check_force allowance 1e-5 max(|F_i|, A_i) + ATOL (exposure left
    out: it only makes the allowance larger for the few exposed rows, which are not counted as powered)."""
    prm, stock = O.OracleParams.from_config(cfg), O.OracleParams.from_config(stock_cfg)
    n = sc.n
    n_t = (n + 63) // 64
    tile = np.arange(n) // 64
    lo = np.array([sc.loc[tile == t, :2].min(axis=0) for t in range(n_t)])
    hi = np.array([sc.loc[tile == t, :2].max(axis=0) for t in range(n_t)])
    vmax = np.array([np.linalg.norm(sc.vel[tile == t], axis=1).max() for t in range(n_t)])
    gap = np.maximum(0.0, np.maximum(lo[:, None, :] - hi[None, :, :], lo[None, :, :] - hi[:, None, :]))
    dist = np.linalg.norm(gap, axis=2)
    reach = stock.ped.gamma * 41.0 * np.log(2.0) * (1.0 + stock.ped.lam * (vmax[:, None] + vmax[None, :]))
    if prm.use_ped_radius:
        reach = reach + 2.0 * sc.radius.max()
    dropped_tiles = dist > reach                                        # (n_t, n_t)
    i0, i1 = rows
    power, allow = np.zeros(i1 - i0), np.zeros(i1 - i0)
    with np.errstate(all="ignore"):
        diff = sc.loc[None, :, :] - sc.loc[i0:i1, None, :]
        e, d = O.unit_and_norm(diff)
        if prm.use_ped_radius:
            d = d - (sc.radius[i0:i1, None] + sc.radius[None, :])
        f, _, _ = O.moussaid_term(e, d, sc.vel[i0:i1, None, :] - sc.vel[None, :, :], prm.ped, 0.0, True)
        mag = np.linalg.norm(f, axis=2)
        mag[np.arange(i1 - i0), np.arange(i0, i1)] = 0.0
        F, _, absum = O.pedestrian_force(sc.loc, sc.vel, sc.radius, prm.ped, prm.use_ped_radius, rows=(i0, i1))
    power = np.where(dropped_tiles[tile[i0:i1]][:, tile], np.nan_to_num(mag), 0.0).sum(axis=1)
    allow = P.RTOL * np.maximum(np.linalg.norm(F, axis=1), absum) + P.ATOL
    return power, allow


def set_config(name, forces, rad=False, readback=False):
    """Set ``name``'s config; ``readback``: max_speed_factor READBACK_MSF for a dt = 1 force read-back (check_force_from_velocity
    asserts that no row comes within a factor of 10 of the cap: at shortrange with use_ped_radius a pedestrian inside a border
    sample's radius feels a exp(+r / b) ~ 1e5 m/s^2)."""
    cfg = psets.config(name, forces, use_ped_radius=rad)
    if readback:
        cfg["max_speed_factor"] = READBACK_MSF
    return cfg
