"""Crowds of ISOLATED ENCOUNTERS, and the kernels' index maps (tests/test_encounters_host.py on the CPU, tests/test_encounters_gpu.py
on the GPU).  No GPU code here.

Every other parity test compares a SUM per pedestrian: 1e-5 of max(|F_i|, A_i) with A_i over all of the row's terms, in crowds whose
near neighbours sit at a few fixed index offsets.  A slot of a kernel -- the place where one pair's term is evaluated and added: tile
shift, rotation, wave, chain, LDS half, ordered row, j-slice -- that is wrong by 1e-3 of its own term passes all of them.  Here every
pedestrian has exactly ONE partner (a perfect matching of the indices) and pair k sits alone at site k of a 100 m lattice: the
row's force IS the partner's term, the partner's index decides the slot, and ``_parity.check_force`` (unchanged) bounds that one term.

``isolated_pairs(n, matching, seed, z_spread)``
  * matching = s (int): i <-> i + s for i in the blocks [2ks, 2ks + s); "random": a seeded permutation paired up; rows left over
    are parked alone on sites of their own.  Pair m of a matching always takes ENCOUNTER m of the set (n // 2 encounters drawn from
    ``seed`` and ``z_spread`` alone) at site m: two matchings of one crowd hold the same pairs of states at different indices.
  * isolation is asserted from the oracle, once per encounter set and on a superset of every crowd built from it (all encounters and
    all parking sites): the float64 sum of |f_ij| over ALL non-partners (``O.moussaid_term``) is <= 1e-9 of the partner's term for
    every row whose term reaches QUALIFY_TERM (the rows the per-term claim is made for), and <= 1e-12 m/s^2 -- a thousandth of
    ``_parity.ATOL`` -- for every row whatever its own term.  (A row's own term can be arbitrarily small -- exp(-d / B) with B -> 0 --
    so no bound relative to it can hold for every row.)
  * all coordinates are fp32-representable; site 0 is the origin, so the designed encounters (which take the first sites) sit on
    small multiples of 100 m and their offsets, all dyadic, survive the addition exactly.

Sampling.  Half of the encounters are drawn as the plain recipe says: distance log-uniform in [0.3, 3] m, bearing uniform, both speeds
uniform in [0, 1.6] m/s with uniform headings, radii uniform in [0.2, 0.45]; with ``z_spread`` heights uniform in [0, z_spread] and
v_z ~ N(0, 0.05).  That recipe alone leaves most cells of the bin grid (below) without a qualifying row -- a pair walking apart has a
term of 1e-10 m/s^2 -- so the other half is STRATIFIED: dealt round-robin to the 48 bins, drawn uniformly inside the bin (angle in
the octant, distance log-uniform in the band, |D| uniform in [0.25, 2] or [2, 5]; the relative velocity (D - e) / lambda is split
between the two pedestrians around a random common velocity so that both speeds stay <= 1.6 m/s), and of up to 40 draws the first
whose float64 term would qualify is kept (``_draw_stratified`` says what happens where that is not enough).  The oracle decides; no kernel is consulted.

Bins: 8 octants of the angle between e and t (wrapped to [-pi, pi)), x 3 distance bands (0.3-0.7, 0.7-1.5, 1.5-3 m), x 2 bands of |D|
(below / from 2).  ``feasible_bins(use_ped_radius)`` evaluates the oracle's term on a dense grid of every bin: in six of the 48 bins
(1, 3, 5, 43, 45, 47: |D| >= 2 with the partner behind, beyond +-3 pi / 4) NO grid point qualifies -- exp(-(n B theta)^2) <= exp(-10.8)
there and the largest term is 2.1e-4 m/s^2, below QUALIFY_TERM -- and no sampling can fill them.  Every other bin must hold at least
4 qualifying rows in every crowd of >= 1024 pairs (measured: >= 19), these six at least 4 checked (paired) rows.  Bins 11 and 41
(1.5-3 m, |D| >= 2, the partner abeam) qualify on ~0.1 % of their volume only; ``_draw_stratified`` draws them from that sliver.

Designed encounters replace the first pairs (each exact in fp32; partner of the first row at (+d, 0) unless said otherwise):
  a  B = 0: D = lambda dv + e = 0 with d = 1 and d = 2 (v_self - v_other = (-1 / lambda, 0)): the reference's term is exactly 0, the
     fast bodies produce NaN and rely on the EXACT recompute;
  b  relative velocity exactly along +e and along -e (theta at 0 / at the +-pi wrap: the oracle's exposure covers both), d = 0.5, 2;
  c  radii against the gap: overlapping (d - r_i - r_j < 0) and touching (= 0 exactly);
  d  3-D crowds only: a partner 2^-10 m off the vertical, and a steep pair with |dz| = 10 |d_xy|;
  e  a pair at rest (dv = 0, D = e).

Reference-alone check of the tolerance (tests/test_encounters_host.py): the partner's term once more by the plain formula in NumPy
float32 must stay within HALF of check_force's allowance of the float64 term on every qualifying row.  Worst ratio seen over the
crowds below: 0.44, and 0.59 with the two norms up to one ulp off (what a 1-ulp reciprocal square root is entitled to; asserted <= 1).
One band is left out: draws whose D_xy cancels by more than a factor of 64 (``encounter_set`` says why).
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import _parity as P
from carla_social_force_model_amd import scenarios
from oracle import sfm_oracle as O

SITE = 100.0                  # m between sites: at gamma 0.35, lambda 2, speeds <= 1.6 (B <= 2.6) a foreign term is < exp(-38) A
QUALIFY_TERM = 1e-3           # m/s^2: ATOL = 1e-9 is then <= 1e-6 of the term and cannot decide a verdict
MAX_WEIGHT = 1.0              # conditioning weight absum / plain - 1 of a qualifying row
MIN_PER_BIN = 4
D_EDGES = (0.3, 0.7, 1.5, 3.0)
DN_SPLIT = 2.0
N_BINS = 8 * 3 * 2
PARK = 192                    # parking sites of an encounter set (rows without a partner)
STOCK = O.Interaction()       # the stock pedestrian_force table (default_sfm_config): the crowds are built for it
R_MAX = 0.45
MAX_KAPPA = 64.0             # largest cancellation factor of D_xy a drawn encounter may have (encounter_set)

_f32 = scenarios._f32


# ---- one encounter in float64 -------------------------------------------------------------------------------------------------------
def pair_terms(loc_a, vel_a, rad_a, loc_b, vel_b, rad_b, use_ped_radius, p=STOCK, theta_tol=0.0):
    """The term on A from B by the oracle (forces.py:74-115 through ``O.moussaid_term``), vectorised over pairs.
    Returns dict: F (k,3), norm, plain (= |f_v| + |f_theta|), weight (conditioned magnitude / plain - 1), expo, phi (angle between
    e and t), d (centre distance, radii not taken off), Dn (|D|)."""
    diff = loc_b - loc_a
    e, d = O.unit_and_norm(diff)
    dist = d - (rad_a + rad_b) if use_ped_radius else d
    dv = vel_a - vel_b
    with np.errstate(all="ignore"):
        F, expo, mag = O.moussaid_term(e, dist, dv, p, theta_tol, True)
        D = p.lam * dv + e
        t, Dn = O.unit_and_norm(D)
        phi, _ = O.wrapped_angle_diff(e, t)
        f_v = np.sum(F * t, axis=-1)
        nrm = np.stack([-t[..., 1], t[..., 0], np.zeros_like(Dn)], axis=-1)
        f_t = np.sum(F * nrm, axis=-1)
        plain = np.abs(f_v) + np.abs(f_t)
        weight = np.where(plain > 0, mag / np.where(plain > 0, plain, 1.0) - 1.0, 0.0)
    return {"F": F, "norm": np.linalg.norm(F, axis=-1), "plain": plain, "weight": weight, "expo": expo, "phi": phi, "d": d, "Dn": Dn}


def bin_of(phi, d, Dn):
    """Bin index octant * 6 + distance band * 2 + |D| band, -1 outside the grid (d outside [0.3, 3], NaN)."""
    phi, d, Dn = np.asarray(phi, float), np.asarray(d, float), np.asarray(Dn, float)
    with np.errstate(invalid="ignore"):
        octant = np.clip(np.floor((phi + np.pi) / (np.pi / 4.0)), 0, 7)
        band = np.digitize(d, D_EDGES) - 1
        ok = (band >= 0) & (band <= 2) & np.isfinite(phi) & np.isfinite(Dn)
        out = octant * 6 + np.clip(band, 0, 2) * 2 + (Dn >= DN_SPLIT)
    return np.where(ok, np.nan_to_num(out), -1).astype(np.int64)


def _bin_box(b):
    octant, band, hi = b // 6, (b % 6) // 2, b % 2
    return (-np.pi + octant * np.pi / 4, -np.pi + (octant + 1) * np.pi / 4), (D_EDGES[band], D_EDGES[band + 1]), ((DN_SPLIT, 5.0) if hi else (0.25, DN_SPLIT))


def _states(phi, d, Dn, beta, ez=0.0, dvz=0.0, p=STOCK):
    """Pair states with angle ``phi`` between e and t (x / y components, as the reference measures it), centre distance d, |D| = Dn and
    bearing beta; ``ez`` the z component of e, ``dvz`` the relative vertical velocity.  Returns (offset of B (k,3), dv (k,3))."""
    ez, dvz = np.broadcast_to(ez, d.shape), np.broadcast_to(dvz, d.shape)
    exy = np.sqrt(np.maximum(0.0, 1.0 - ez * ez))
    e = np.stack([exy * np.cos(beta), exy * np.sin(beta), ez], axis=-1)
    Dz = p.lam * dvz + ez
    Dxy = np.sqrt(np.maximum(1e-6, Dn * Dn - Dz * Dz))
    D = np.stack([Dxy * np.cos(beta - phi), Dxy * np.sin(beta - phi), Dz], axis=-1)
    return d[..., None] * e, (D - e) / p.lam


def _acceptable(t):
    """What the stratified draws aim for: a term of 1.5 QUALIFY_TERM, a conditioning weight of 0.5 MAX_WEIGHT, no exposure.  (The weight:
    with draws up to 0.8 one encounter -- |D| = 4.3, angle 0.9, weight 0.56 -- put the plain float32 formula at 0.57 of the allowance, above
    the half that tests/test_encounters_host.py asks for; the stratified draws therefore stay at half the qualifying weight.)"""
    return (t["norm"] >= 1.5 * QUALIFY_TERM) & (t["weight"] <= 0.5 * MAX_WEIGHT) & (np.nan_to_num(t["expo"]) == 0.0)


def _qualifies(t):
    return (t["norm"] >= QUALIFY_TERM) & (t["weight"] <= MAX_WEIGHT) & (np.nan_to_num(t["expo"]) == 0.0)


@functools.lru_cache(maxsize=None)
def feasible_bins(use_ped_radius):
    """Per bin: can the oracle's formula hold a qualifying term anywhere in it?  A dense grid -- angle 32 points across the octant, |D|
    25 points, d 9 points across the band (log-spaced), planar, radii (use_ped_radius) 0.2 .. R_MAX in 3 steps each way -- evaluated
    by ``pair_terms``.  Returns (largest term[48], share of the grid points that qualify[48], feasible[48]): a bin is infeasible
    only when NO grid point qualifies -- bins 1, 3, 5, 43, 45, 47, whose largest term is 2.1e-4 m/s^2, below QUALIFY_TERM."""
    best, share = np.zeros(N_BINS), np.zeros(N_BINS)
    radii = (0.2, 0.325, R_MAX) if use_ped_radius else (0.2,)
    for b in range(N_BINS):
        (p0, p1), (d0, d1), (n0, n1) = _bin_box(b)
        phi, Dn, d, ra, rb = (a.ravel() for a in np.meshgrid(np.linspace(p0, p1, 33)[:-1] + 1e-9, np.linspace(n0, n1, 25),
                                                              np.exp(np.linspace(np.log(d0), np.log(d1), 9)), radii, radii, indexing="ij"))
        lb, va = _states(phi, d, Dn, np.zeros_like(phi))
        za = np.zeros((len(phi), 3))
        t = pair_terms(za, va, ra, lb, za, rb, use_ped_radius, theta_tol=50 * P.THETA_TOL)
        best[b], share[b] = np.nanmax(t["norm"]), _qualifies(t).mean()
    return best, share, share > 0.0


# ---- an encounter set ------------------------------------------------------------------------------------------------------------------
def _designed(z_spread):
    """[(label, offset of B (3), v_A (3), v_B (3), r_A, r_B)]: all values dyadic.  A set of P encounters takes the first P // 8 of
    the list (a crowd of 32 pairs: four of them), so that half of a small crowd's rows can still qualify."""
    lam = STOCK.lam
    out = [("a:B=0,d=1", (1.0, 0, 0), (-0.25, 0.5, 0), (-0.25 + 1.0 / lam, 0.5, 0), 0.25, 0.3125),
           ("e:rest", (0.0, 1.0, 0), (0, 0, 0), (0, 0, 0), 0.25, 0.25),
           ("c:touch", (0.625, 0, 0), (0.25, -0.5, 0), (0.5, 0.25, 0), 0.3125, 0.3125),
           ("b:+e,d=0.5", (0.5, 0, 0), (0.75, 0.25, 0), (0.25, 0.25, 0), 0.25, 0.25),
           ("a:B=0,d=2", (2.0, 0, 0), (0.125, -0.25, 0), (0.125 + 1.0 / lam, -0.25, 0), 0.375, 0.25),
           ("b:-e,d=0.5", (0.5, 0, 0), (-0.5, 0.25, 0), (0.5, 0.25, 0), 0.25, 0.25),
           ("c:overlap", (0.5, 0, 0), (0.5, 0.25, 0), (-0.25, 0.5, 0), 0.3125, 0.3125),
           ("b:+e,d=2", (2.0, 0, 0), (0.5, -0.5, 0), (0.0, -0.5, 0), 0.3125, 0.25),
           ("b:-e,d=2", (2.0, 0, 0), (-0.25, 0.5, 0), (0.75, 0.5, 0), 0.25, 0.375)]
    if z_spread:
        out[3:3] = [("d:near-vertical", (2.0 ** -10, 0, 1.0), (0.5, 0.25, 0.0625), (-0.25, 0.5, 0), 0.25, 0.25),
                    ("d:steep", (0.0625, 0, 0.625), (0.25, 0.5, 0), (0.5, -0.25, -0.0625), 0.25, 0.25)]
    return out


@dataclass
class EncounterSet:
    """P encounters (A and B of pair m at site m) and PARK lone pedestrians on sites of their own."""
    loc: np.ndarray            # (P, 2, 3) absolute, fp32-representable
    vel: np.ndarray            # (P, 2, 3)
    rad: np.ndarray            # (P, 2)
    park_loc: np.ndarray       # (PARK, 3)
    park_vel: np.ndarray
    park_rad: np.ndarray
    labels: dict = field(default_factory=dict)      # designed label -> pair index


def _sites(k, layout):
    """Site k of the lattice.  'lattice': row-major on a square, rows 64 sites long at most.  'blocks': 8 x 8 blocks of sites, block after
    block along x -- 64 consecutive sites share a 700 m box and the next 64 lie >= 100 m away (the list cutoff's reach at the stock
    parameters is 74 m: gamma 41 ln2 (1 + lambda 3.2))."""
    k = np.asarray(k)
    if layout == "blocks":
        blk, w = k // 64, k % 64
        return np.stack([(blk * 8 + w % 8) * SITE, (w // 8) * SITE, np.zeros(k.shape)], axis=-1)
    return np.stack([(k % 64) * SITE, (k // 64) * SITE, np.zeros(k.shape)], axis=-1)


def _draw_dz(rng, d, z_spread):
    """Height difference of a pair: two heights uniform in [0, z_spread], their difference held to 0.8 d so that d stays the
    (log-uniform) centre distance.  Returns (z_A, dz)."""
    k = len(d)
    if not z_spread:
        return np.zeros(k), np.zeros(k)
    za, zb = rng.uniform(0.0, z_spread, k), rng.uniform(0.0, z_spread, k)
    return za, np.clip(zb - za, -0.8 * d, 0.8 * d)


def _draw_plain(rng, k, z_spread):
    d = np.exp(rng.uniform(np.log(0.3), np.log(3.0), k))
    beta = rng.uniform(-np.pi, np.pi, k)
    za, dz = _draw_dz(rng, d, z_spread)
    dxy = np.sqrt(d * d - dz * dz)
    off = np.stack([dxy * np.cos(beta), dxy * np.sin(beta), dz], axis=-1)
    vel = np.zeros((k, 2, 3))
    for s in (0, 1):
        sp, hd = rng.uniform(0.0, 1.6, k), rng.uniform(-np.pi, np.pi, k)
        vel[:, s, 0], vel[:, s, 1] = sp * np.cos(hd), sp * np.sin(hd)
        if z_spread:
            vel[:, s, 2] = rng.normal(0.0, 0.05, k)
    return off, vel, za


def _candidates(rng, lo, hi, z_spread):
    """One uniform draw inside each box of (angle, log d, |D|) ``lo`` .. ``hi``: (offset of B, velocities (k,2,3), z_A, acceptable)."""
    k = len(lo)
    unit = lambda a: np.stack([np.cos(a), np.sin(a)], axis=-1)
    q = lo + rng.uniform(0.02, 0.98, (k, 3)) * (hi - lo)
    phi, d, Dn = q[:, 0], np.exp(q[:, 1]), q[:, 2]
    z_a, dz = _draw_dz(rng, d, z_spread)
    vz = rng.normal(0.0, 0.05, (k, 2)) if z_spread else np.zeros((k, 2))
    o3, dv = _states(phi, d, Dn, rng.uniform(-np.pi, np.pi, k), dz / d, vz[:, 0] - vz[:, 1])
    room = np.maximum(0.0, 1.6 - 0.5 * np.linalg.norm(dv[:, :2], axis=1)) * 0.9
    c = (room * np.sqrt(rng.uniform(0, 1, k)))[:, None] * unit(rng.uniform(-np.pi, np.pi, k))
    v = np.zeros((k, 2, 3))
    v[:, 0, :2], v[:, 1, :2] = c + 0.5 * dv[:, :2], c - 0.5 * dv[:, :2]
    v[:, :, 2] = vz
    zero, r = np.zeros((k, 3)), np.full(k, 0.2)               # (the smallest radii: larger ones only raise the term)
    good, score = np.ones(k, bool), np.full(k, np.inf)
    for rad in (False, True):
        t = pair_terms(zero, v[:, 0], r, o3, v[:, 1], r, rad, theta_tol=50 * P.THETA_TOL)
        good &= _acceptable(t)
        score = np.minimum(score, np.where((t["weight"] <= 0.5 * MAX_WEIGHT) & (np.nan_to_num(t["expo"]) == 0.0), np.nan_to_num(t["norm"]), 0.0))
    return o3, v, z_a, good, score, q


def _draw_stratified(rng, bins, z_spread, tries=40, pool=20000):
    """One encounter per entry of ``bins``, drawn uniformly inside the bin: of up to ``tries`` draws the first whose float64 term
    qualifies (both radius settings, weight and exposure included, with a margin of 1.5 on the term) is kept.  A bin of which only a
    sliver qualifies (0.1 % of bins 11 and 41: 1.5-3 m, |D| >= 2, the partner abeam) does not get there; its entries are then taken
    from the qualifying ones among ``pool`` further draws of that bin, the box of the draws shrinking onto the best 2 % of the previous
    round until enough qualify.  Where nothing qualifies (the six bins that cannot hold a qualifying term at all) the last draw is kept."""
    k = len(bins)
    off, vel, za = np.zeros((k, 3)), np.zeros((k, 2, 3)), np.zeros(k)
    done = np.zeros(k, bool)
    boxes = [_bin_box(b) for b in bins]
    lo = np.array([[bx[0][0], np.log(bx[1][0]), bx[2][0]] for bx in boxes]).reshape(k, 3)
    hi = np.array([[bx[0][1], np.log(bx[1][1]), bx[2][1]] for bx in boxes]).reshape(k, 3)
    for attempt in range(tries):
        o3, v, z_a, good, _, _ = _candidates(rng, lo, hi, z_spread)
        take = ~done & good
        off[take], vel[take], za[take] = o3[take], v[take], z_a[take]
        done |= take
    left = ~done
    off[left], vel[left], za[left] = o3[left], v[left], z_a[left]
    for b in np.unique(np.asarray(bins)[left]):
        rows = np.nonzero(left & (np.asarray(bins) == b))[0]
        blo, bhi = lo[rows[0]].copy(), hi[rows[0]].copy()
        for _ in range(5):                                   # the box shrinks onto the best 2 % of its draws until enough of them qualify
            o3, v, z_a, good, score, q = _candidates(rng, np.repeat(blo[None], pool, axis=0), np.repeat(bhi[None], pool, axis=0), z_spread)
            if good.sum() >= len(rows) or score.max() < QUALIFY_TERM:
                break
            top = q[np.argsort(-score)[:pool // 50]]
            blo, bhi = top.min(axis=0), top.max(axis=0)
        hits = np.nonzero(good)[0][:len(rows)]
        rows = rows[:len(hits)]
        off[rows], vel[rows], za[rows] = o3[hits], v[hits], z_a[hits]
    return off, vel, za


@functools.lru_cache(maxsize=None)
def encounter_set(n_pairs, seed, z_spread=0.0, layout="lattice"):
    rng = np.random.default_rng(seed)
    P_ = n_pairs
    n_plain = P_ // 2
    off, vel, za = np.zeros((P_, 3)), np.zeros((P_, 2, 3)), np.zeros(P_)
    off[:n_plain], vel[:n_plain], za[:n_plain] = _draw_plain(rng, n_plain, z_spread)
    bins = (np.arange(P_ - n_plain) + seed) % N_BINS
    if P_ > n_plain:
        off[n_plain:], vel[n_plain:], za[n_plain:] = _draw_stratified(rng, bins, z_spread)
    order = rng.permutation(P_)                       # plain and stratified encounters interleaved over the indices
    off, vel, za = off[order], vel[order], za[order]
    rad = rng.uniform(0.2, R_MAX, (P_, 2))
    # A band that is left out: D_xy = lambda dv_xy + e_xy may cancel
    # while D_z keeps |D|, B and the term finite.  The angle of t is then the angle of a difference of O(1) numbers, resolved in fp32
    # only to kappa 2^-23 rad, kappa = (lambda |dv_xy| + |e_xy|) / |D_xy| -- the reference's own conditioning, which the conditioning
    # weight of the tolerance (2^-22 rad of angle noise) does not know.  A 3-D draw with kappa = 1714 put the plain float32 formula
    # with its norms one ulp off at 2.2 of the allowance; every other draw of every set stays below 0.7.  Draws with kappa > 64 are
    # drawn again by the plain recipe (last in the generator's stream, so the other sets are unchanged).
    for _ in range(20):
        dv = vel[:, 0] - vel[:, 1]
        e, _d = O.unit_and_norm(off)
        Dxy = np.linalg.norm(STOCK.lam * dv[:, :2] + e[:, :2], axis=1)
        kappa = (STOCK.lam * np.linalg.norm(dv[:, :2], axis=1) + np.linalg.norm(e[:, :2], axis=1)) / np.maximum(Dxy, 1e-300)
        again = np.nonzero(kappa > MAX_KAPPA)[0]
        if not len(again):
            break
        off[again], vel[again], za[again] = _draw_plain(rng, len(again), z_spread)
    labels = {}
    for m, (label, o, va, vb, ra, rb) in enumerate(_designed(z_spread)[:P_ // 8]):
        off[m], vel[m, 0], vel[m, 1], rad[m], za[m] = o, va, vb, (ra, rb), 0.0
        labels[label] = m
    site = _sites(np.arange(P_), layout)
    loc = np.zeros((P_, 2, 3))
    loc[:, 0] = site + np.stack([np.zeros(P_), np.zeros(P_), za], axis=-1)
    loc[:, 1] = loc[:, 0] + off
    park_loc = _sites(P_ + np.arange(PARK), layout)
    sp, hd = rng.uniform(0.0, 1.6, PARK), rng.uniform(-np.pi, np.pi, PARK)
    park_vel = np.stack([sp * np.cos(hd), sp * np.sin(hd), np.zeros(PARK)], axis=-1)
    if z_spread:
        park_loc[:, 2] = rng.uniform(0.0, z_spread, PARK)
        park_vel[:, 2] = rng.normal(0.0, 0.05, PARK)
    es = EncounterSet(_f32(loc), _f32(vel), _f32(rad), _f32(park_loc), _f32(park_vel), _f32(rng.uniform(0.2, R_MAX, PARK)), labels)
    _assert_isolated(es)
    return es


def _assert_isolated(es, chunk=128):
    """From the oracle, not from the lattice constant: per row of the SUPERSET (every encounter, every parking site) the float64 sum
    of |f_ij| over all non-partners against the partner's term.  One evaluation bounds both radius settings: a term's magnitude
    A exp(-dist / B) g(B, theta) falls with dist, so dist = d - 2 R_MAX is an upper bound for any radii and for none; and
    |f_ij| = |f_ji| (D, e change sign together: B and theta are the same), so every unordered pair is evaluated once."""
    P_ = len(es.loc)
    loc = np.concatenate([es.loc.reshape(-1, 3), es.park_loc])
    vel = np.concatenate([es.vel.reshape(-1, 3), es.park_vel])
    n = len(loc)
    partner = np.concatenate([np.arange(2 * P_) ^ 1, np.full(PARK, -1)])
    idx = np.arange(n)
    foreign = np.zeros(n)
    for s in range(0, n, chunk):
        e_ = min(n, s + chunk)
        e, d = O.unit_and_norm(loc[None, s:, :] - loc[s:e_, None, :])
        with np.errstate(all="ignore"):
            f, _, _ = O.moussaid_term(e, d - 2.0 * R_MAX, vel[s:e_, None, :] - vel[None, s:, :], STOCK, 0.0, False)
        mag = np.linalg.norm(f, axis=2)
        skip = (idx[None, s:] <= idx[s:e_, None]) | (idx[None, s:] == partner[s:e_, None])
        mag = np.where(skip, 0.0, np.nan_to_num(mag))
        foreign[s:e_] += mag.sum(axis=1)
        foreign[s:] += mag.sum(axis=0)
    assert foreign.max() <= 1e-12, f"foreign terms up to {foreign.max():.3e} m/s^2"
    a, b = es.loc.reshape(-1, 3), es.loc[:, ::-1].reshape(-1, 3)
    for use_rad in (False, True):
        own = np.nan_to_num(pair_terms(a, es.vel.reshape(-1, 3), es.rad.reshape(-1), b, es.vel[:, ::-1].reshape(-1, 3),
                                       es.rad[:, ::-1].reshape(-1), use_rad)["norm"])
        used = own >= QUALIFY_TERM
        assert (foreign[:2 * P_][used] <= 1e-9 * own[used]).all(), "a qualifying row is not isolated"


# ---- crowds ----------------------------------------------------------------------------------------------------------------------------
def matching_pairs(n, matching, seed):
    """[(i, j)] in pair order, i = side A.  int s: i <-> i + s for i in [2ks, 2ks + s), both below n; 'random': a permutation of
    the indices from ``seed`` ("random-K": from seed + K), paired up two by two."""
    if isinstance(matching, str):                           # "random", or "random-K": another permutation
        p = np.random.default_rng(seed + 99991 + int(matching[7:] or 0)).permutation(n)
        return np.stack([p[0:n - n % 2:2], p[1:n:2]], axis=1)
    s = int(matching)
    i = np.arange(n)
    i = i[((i // s) % 2 == 0) & (i + s < n)]
    return np.stack([i, i + s], axis=1)


@dataclass
class Crowd:
    sc: scenarios.Scenario
    partner: np.ndarray        # (n,) partner's index, -1: parked alone
    pair: np.ndarray           # (n,) encounter index, -1
    side: np.ndarray           # (n,) 0 = A, 1 = B
    designed: dict             # label -> (row of A, row of B)
    n_pairs: int

    @property
    def paired(self):
        return self.partner >= 0

    def ident(self):
        """Row -> identity of the pedestrian across matchings: 2 * encounter + side (parked rows: -1)."""
        return np.where(self.paired, 2 * self.pair + self.side, -1)


@functools.lru_cache(maxsize=None)
def isolated_pairs(n, matching, seed, z_spread=0.0, layout="lattice"):
    es = encounter_set(n // 2, seed, z_spread, layout)
    pairs = matching_pairs(n, matching, seed)
    loc, vel, rad = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    partner, pair, side = np.full(n, -1), np.full(n, -1), np.zeros(n, dtype=np.int64)
    for s in (0, 1):
        r = pairs[:, s]
        m = np.arange(len(pairs))
        loc[r], vel[r], rad[r] = es.loc[m, s], es.vel[m, s], es.rad[m, s]
        partner[r], pair[r], side[r] = pairs[:, 1 - s], m, s
    alone = np.nonzero(partner < 0)[0]
    assert len(alone) <= PARK, (n, matching, len(alone))
    loc[alone], vel[alone], rad[alone] = es.park_loc[:len(alone)], es.park_vel[:len(alone)], es.park_rad[:len(alone)]
    wp = loc.copy()
    wp[:, 0] += 10.0
    wp[:, 2] = 0.0
    sc = scenarios.Scenario(loc=loc, vel=vel, waypoint=_f32(wp), target_speed=_f32(np.full(n, 1.2)), radius=rad,
                            mode=np.ones(n, dtype=np.int64), world_side=float(np.float32(loc[:, :2].max() + SITE)), seed=seed)
    designed = {k: (int(pairs[m, 0]), int(pairs[m, 1])) for k, m in es.labels.items() if m < len(pairs)}
    return Crowd(sc, partner, pair, side, designed, len(pairs))


# ---- the oracle's side of a cell ---------------------------------------------------------------------------------------------------------
PED_ONLY = ("pedestrian_force",)


@dataclass
class CellRef:
    F: np.ndarray              # (n,3) pedestrian force, C oracle
    expo: np.ndarray
    absum: np.ndarray
    plain: np.ndarray
    term: np.ndarray           # |F_i|
    weight: np.ndarray
    qualifying: np.ndarray     # bool (n,)
    bins: np.ndarray           # (n,) bin of the row's encounter, -1
    v_new: np.ndarray
    use_ped_radius: bool = False


_REF_CACHE = {}


def reference(crowd, cfg, dt=1.0, geom=None):
    """One C-oracle tick of ``crowd`` under ``cfg`` (pedestrian force, optionally a border force no row keeps); kept per crowd and
    configuration (the crowds themselves are kept by ``isolated_pairs``), since several tests ask for the same tick."""
    key = (id(crowd), repr(cfg), dt) if geom is None else None
    if key in _REF_CACHE:
        return _REF_CACHE[key]
    ref = _reference(crowd, cfg, dt, geom)
    if key is not None:
        _REF_CACHE[key] = ref
    return ref


def _reference(crowd, cfg, dt, geom):
    from oracle import c_oracle
    sc = crowd.sc
    prm = O.OracleParams.from_config(cfg)
    plain = np.zeros(sc.n)
    with np.errstate(all="ignore"):
        per, total, v_new, expo, absum = c_oracle.tick(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, np.zeros(sc.n, bool),
                                                       O.Geometry() if geom is None else geom, prm, dt, theta_tol=P.THETA_TOL, plain=plain)
    F = per["pedestrian_force"]
    term = np.linalg.norm(F, axis=1)
    weight = np.nan_to_num(np.where(plain > 0, absum / np.where(plain > 0, plain, 1.0) - 1.0, 0.0), nan=np.inf)
    q = crowd.paired & (term >= QUALIFY_TERM) & (np.nan_to_num(expo) == 0.0) & (weight <= MAX_WEIGHT)
    pr = np.where(crowd.paired, crowd.partner, 0)
    t = pair_terms(sc.loc, sc.vel, sc.radius, sc.loc[pr], sc.vel[pr], sc.radius[pr], prm.use_ped_radius, prm.ped)
    bins = np.where(crowd.paired, bin_of(t["phi"], t["d"], t["Dn"]), -1)
    return CellRef(F, expo, absum, plain, term, weight, q, bins, v_new, bool(prm.use_ped_radius))


def bin_counts(ref, rows=None):
    """(qualifying rows per bin, paired rows per bin) over ``rows`` (default: all)."""
    sel = np.ones(len(ref.bins), bool) if rows is None else rows
    b = ref.bins
    return (np.bincount(b[sel & ref.qualifying & (b >= 0)], minlength=N_BINS), np.bincount(b[sel & (b >= 0)], minlength=N_BINS))


def assert_bins(label, ref):
    """Every feasible bin holds >= MIN_PER_BIN qualifying rows, every other bin that many checked rows."""
    feasible = feasible_bins(bool(ref.use_ped_radius))[2]
    q, allr = bin_counts(ref)
    short = [b for b in range(N_BINS) if (q[b] if feasible[b] else allr[b]) < MIN_PER_BIN]
    assert not short, f"{label}: bins {short} hold {[int(q[b]) for b in short]} qualifying / {[int(allr[b]) for b in short]} rows"
    return q, allr


def plain_float32_term(crowd, use_ped_radius, p=STOCK, nudge=(0, 0)):
    """The partner's term by the plain formula (forces.py:74-115 step by step: difference, normalise, D, normalise, two arctan2 and one
    wrap, B, theta, the two exponentials, f_v t + f_theta n) with every operation in NumPy float32 -- no kernel trick, no fma, no
    folded constant.  What ANY straightforward fp32 evaluation is entitled to.  ``nudge`` = (k_d, k_D): the two norms |diff| and |D| off
    by that many ulps, which is what an evaluation through a 1-ulp reciprocal square root is entitled to as well."""
    f = np.float32
    sc = crowd.sc
    pr = np.where(crowd.paired, crowd.partner, 0)
    la, lb, va, vb = (np.asarray(a, dtype=f) for a in (sc.loc, sc.loc[pr], sc.vel, sc.vel[pr]))
    ra, rb = np.asarray(sc.radius, dtype=f), np.asarray(sc.radius[pr], dtype=f)
    with np.errstate(all="ignore"):
        diff = lb - la
        d = np.sqrt(np.sum(diff * diff, axis=1, dtype=f), dtype=f) * f(1.0 + nudge[0] * 2.0 ** -23)
        e = diff / np.where(d == 0, f(1), d)[:, None]
        dist = d - (ra + rb) if use_ped_radius else d
        D = f(p.lam) * (va - vb) + e
        Dn = np.sqrt(np.sum(D * D, axis=1, dtype=f), dtype=f) * f(1.0 + nudge[1] * 2.0 ** -23)
        t = D / np.where(Dn == 0, f(1), Dn)[:, None]
        ang = np.arctan2(e[:, 1], e[:, 0]) - np.arctan2(t[:, 1], t[:, 0])
        ang = np.where(ang > f(np.pi), ang - f(2 * np.pi), ang)
        ang = np.where(ang < f(-np.pi), ang + f(2 * np.pi), ang)
        B = f(p.gamma) * Dn
        theta = ang + B * f(-p.epsilon)
        f_v = f(-p.A) * np.exp(f(-1.0) * dist / B - np.square(f(p.n_prime) * B * theta))
        f_t = f(-p.A) * np.sign(theta) * np.exp(f(-1.0) * dist / B - np.square(f(p.n) * B * theta))
        F = f_v[:, None] * t
        F[:, 0] += f_t * (-t[:, 1])
        F[:, 1] += f_t * t[:, 0]
    assert F.dtype == np.float32
    return np.where(crowd.paired[:, None], F.astype(np.float64), 0.0)


def allowance(ref):
    """check_force's allowance per row (exposure included), _parity.check_force's own expression."""
    scale = np.maximum(ref.term, np.nan_to_num(ref.absum))
    return P.RTOL * scale + np.nan_to_num(ref.expo) * 1.001 + P.ATOL


# ---- the kernels' index maps -------------------------------------------------------------------------------------------------------------
WAVE = 64


def _sigma(l_trav, l_res):
    return (l_trav - l_res) & 63


def slots_symmetric(n, i, j):
    """Where sfm_pair_sym_kernel (csrc/sfm_kernels.hip, pair_block) evaluates the unordered pair {i, j} in grid mode.  Mirrors:
    :1264-1281 the work item -- tiles ta (travelling) and tb = ta + shift (resident), shift <= n_t / 2, the antipodal shift of an even
    n_t by its lower tile only (:1276); a diagonal tile by waves 0, 1 or 2, 3 with sig0 = 1 + 16 (wave & 1) (:1267-1271), else
    sig0 = 16 wave (:1280);  :1312, :1353 lane l of the resident tile meets slot l + sig0 + s_ of the doubled travelling image, i.e.
    travelling lane (l + sigma) & 63 at rotation sigma = sig0 + s_, 16 steps per wave.
    Returns arrays (shift, sigma, wave, step) per pair; on a diagonal tile wave is wave & 1."""
    i, j = np.asarray(i), np.asarray(j)
    n_t = (n + 63) // 64
    ti, tj, li, lj = i // 64, j // 64, i % 64, j % 64
    fwd = (tj - ti) % n_t                                    # tile distance going up from i's tile
    diag = ti == tj
    # off-diagonal: the travelling tile is the one from which the other is at most n_t / 2 ahead (tie: the lower tile)
    i_trav = np.where(2 * fwd < n_t, True, np.where(2 * fwd == n_t, ti < tj, False))
    shift = np.where(diag, 0, np.where(i_trav, fwd, n_t - fwd))
    sig_off = np.where(i_trav, _sigma(li, lj), _sigma(lj, li))
    delta = (lj - li) & 63                                   # diagonal: resident l meets (l + sigma), sigma in 1..32
    sig_diag = np.where(delta <= 32, delta, 64 - delta)
    sigma = np.where(diag, sig_diag, sig_off)
    wave = np.where(diag, (sigma - 1) // 16, sigma // 16)
    step = np.where(diag, (sigma - 1) % 16, sigma % 16)
    return shift, sigma, wave, step


def fused_waves(n, geo):
    """Waves per workgroup of the fused tick: ``fused_launch`` in csrc/sfm_capi.hip (16, or 8 when pair + geometry workgroups exceed 512)."""
    n_t = (n + 63) // 64
    n_g = (n_t + 1) // 2
    n_pair = (n_g + 1) // 2 + n_g * ((n_g - 1) // 2) + (0 if n_g & 1 else n_g // 2)      # sfm_kernels.hip:2497
    if not geo:
        return 16
    slices = 4 if n_t <= 64 else 2
    if n_t >= 6 and n_pair <= 256:                     # (C++ integer division: a negative quotient never wins the max)
        slices = max(slices, min(8, (256 - n_pair) // n_t))
    return 8 if n_pair + n_t * slices > 512 else 16


def slots_fused(n, i, j, nw):
    """Where sfm_fused_tick_kernel evaluates {i, j} (csrc/sfm_kernels.hip).  Tiles go in groups of two (:1815).  Mirrors:
    :1897-1937 the work item (GX, GY): blocked form (n_g % 8 == 0) always with GX < GY, otherwise group pairs (bx, bx + shift) with
    shift <= n_g / 2 (the half shift of an even n_g by its lower half), diagonal items for a group's own pairs;
    :2162-2184 the wave's role -- diagonal tile: D = NW / 8 waves, sig0 = 1 + (lw % D) SPW; tile 0 past tile 1 of a group and
    off-diagonal tile pairs (q = wave / (NW / 4): tile q >> 1 of GX travels past tile q & 1 of GY): NW / 4 waves, sig0 = k SPW;
    :2201-2248 two chains per wave: s0 = sig0 / 2 (diagonal: 1 + (sig0 - 1) / 2), chain A rotations s0 .. s0 + HALF - 1, chain B the
    same XB further on (32; 16 on a diagonal tile), HALF = SPW / 2 = 128 / NW double steps; resident lane l meets travelling lane
    (l + sigma) & 63.
    Returns (kind 0 diagonal tile / 1 inside a group / 2 between groups, tile shift tb - ta mod n_t as the symmetric kernel counts
    it, sigma, wave within the tile pair's waves, chain 0 / 1, double step)."""
    i, j = np.asarray(i), np.asarray(j)
    n_t = (n + 63) // 64
    n_g = (n_t + 1) // 2
    half = 128 // nw
    ti, tj, li, lj = i // 64, j // 64, i % 64, j % 64
    gi, gj = ti // 2, tj // 2
    same_tile, same_group = ti == tj, (gi == gj) & (ti != tj)
    if n_g % 8 == 0:
        i_is_gx = gi < gj
    else:
        fwd = (gj - gi) % n_g
        i_is_gx = np.where(2 * fwd < n_g, True, np.where(2 * fwd == n_g, gi < gj, False))
    # travelling side: tile 0 of a group past tile 1; GX's tile past GY's
    i_trav = np.where(same_group, ti < tj, i_is_gx)
    sig_off = np.where(i_trav, _sigma(li, lj), _sigma(lj, li))
    delta = (lj - li) & 63
    sig_diag = np.where(delta <= 32, delta, 64 - delta)
    sigma = np.where(same_tile, sig_diag, sig_off)
    xb = np.where(same_tile, 16, 32)
    r = np.where(same_tile, sigma - 1, sigma)                 # rotation counted from the tile pair's first
    chain = (r // xb) % 2
    wave = (r % xb) // half
    step = (r % xb) % half
    kind = np.where(same_tile, 0, np.where(same_group, 1, 2))
    shift = np.minimum((tj - ti) % n_t, (ti - tj) % n_t)
    return kind, shift, sigma, wave, chain, step


def slots_ordered(i, j, ipw, team):
    """sfm_tick_kernel<IPW, .., TEAM> (csrc/sfm_kernels.hip): a wave owns IPW consecutive rows (:700, row k = i mod IPW from a shard that
    starts at 0), the lanes span j (:757, lane = j mod 64), TEAM 4: wave w of the workgroup takes the j-tiles 4 s + w (:838-849).
    Returns (row k, team wave, lane) for the term on i from j."""
    i, j = np.asarray(i), np.asarray(j)
    return i % ipw, (j // 64) % team, j % 64


def slots_batch(n, i, j):
    """sfm_batch.hip batch_scene (:163-169): S = 4 / 2 / 1 j-slices for n <= 64 / <= 128 / larger, R = 256 / S rows per pass, chunk =
    ceil(n / S); the term on i from j is evaluated by slice j // chunk in pass i // R (batch_pair_sum, :77).  Returns (S, slice, pass)."""
    i, j = np.asarray(i), np.asarray(j)
    S = 4 if n <= 64 else 2 if n <= 128 else 1
    R, chunk = 256 // S, (n + S - 1) // S
    return S, j // chunk, i // R


# ---- the crowds both test files use ------------------------------------------------------------------------------------------------------
OFFSETS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 1000)


def matchings(n):
    """The partner offsets of a path at size n: OFFSETS below n / 2, n / 2 itself, and one random matching."""
    return [s for s in OFFSETS if s < n // 2] + [n // 2, "random"]


SEED = 4200
# (path, n, z_spread, use_ped_radius, layout): one line per kernel instantiation and size the GPU file runs, each for every matching of
# ``matchings(n)`` (the list path: LIST_MATCHINGS, which keep the tiles compact).  "ordered-I-T": SFM_IPW = I, SFM_TEAM = T.
PATHS = [("fused", 128, 0.0, False, "lattice"), ("fused", 128, 0.0, True, "lattice"),
         ("fused", 4096, 0.0, False, "lattice"), ("fused", 4096, 0.0, True, "lattice"),
         ("fused3d", 256, 1.5, False, "lattice"), ("fused3d", 4096, 1.5, False, "lattice"), ("fused3d", 4096, 1.5, True, "lattice"),
         ("fused3d-geo", 4096, 1.5, True, "lattice"),
         ("sym", 64, 0.0, False, "lattice"), ("sym", 1000, 0.0, True, "lattice"), ("sym", 1000, 1.5, False, "lattice"),
         ("sym", 4096, 0.0, False, "lattice"), ("sym", 4096, 0.0, True, "lattice"), ("sym", 4096, 1.5, False, "lattice"),
         ("sym", 4096, 1.5, True, "lattice"),
         ("ordered-8-4", 257, 0.0, False, "lattice"), ("ordered-1-1", 1024, 0.0, True, "lattice"), ("ordered-8-4", 1024, 0.0, False, "lattice"),
         ("ordered-8-1", 1024, 1.5, True, "lattice"), ("ordered-1-4", 1024, 1.5, False, "lattice"),
         ("list", 2048, 0.0, False, "blocks"), ("list", 2048, 1.5, True, "blocks")]
LIST_MATCHINGS = (1, 33, 64, 128)
# the batch: (rows, matching) per scene -- the j-slices S = 4 / 2 / 1 (rows <= 64 / <= 128 / more) and one to four passes of 256 rows
BATCH_SCENES = ((2, 1), (64, 1), (64, 16), (64, 32), (64, "random"), (128, 1), (128, 64), (128, "random"), (128, "random-1"), (130, 65), (300, "random"),
                (1024, 300))
FULL_COVERAGE_N = 1024        # paths at this size or above must cover every slot class; smaller crowds are there for the ragged ends


def path_matchings(path, n):
    return list(LIST_MATCHINGS) if path == "list" else matchings(n)


def crowd_specs():
    """Every (n, matching, seed, z_spread, layout) the GPU file builds -- the host file checks the oracle-side conditions on all."""
    out = []
    for path, n, z, rad, layout in PATHS:
        out += [(n, m, SEED + n, z, layout) for m in path_matchings(path, n)]
    for z in (0.0, 1.5):
        out += [(n, m, SEED + n, z, "lattice") for n, m in BATCH_SCENES]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def fused_wave_id(n, i, j, nw):
    """The wave of its workgroup that evaluates {i, j} in the fused tick (csrc/sfm_kernels.hip:2162-2184): off-diagonal items
    q (NW / 4) + w with q = 2 (tile of GX & 1) + (tile of GY & 1); diagonal items sel (NW / 2) + lw, sel = 0 for the item's first group
    (:1916 blocked: the even group of a neighbouring pair; :1934-1935 otherwise: the group below half_up), lw = tl D + w on a diagonal
    tile (D = NW / 8 waves), 2 D + w for tile 0 past tile 1."""
    kind, shift, sigma, wave, chain, step = slots_fused(n, i, j, nw)
    i, j = np.asarray(i), np.asarray(j)
    n_t = (n + 63) // 64
    n_g = (n_t + 1) // 2
    ti, tj = i // 64, j // 64
    g = ti // 2
    sel = (g & 1) if n_g % 8 == 0 else (g >= (n_g + 1) // 2)
    D = nw // 8
    diag_id = sel * (nw // 2) + np.where(kind == 0, (ti & 1) * D + wave, 2 * D + wave)
    # between groups: which of the two tiles travels is slots_fused's rule; recover it from sigma
    li, lj = i % 64, j % 64
    i_trav = ((li - lj) & 63) == sigma
    q = np.where(i_trav, 2 * (ti & 1) + (tj & 1), 2 * (tj & 1) + (ti & 1))
    return np.where(kind == 2, q * (nw // 4) + wave, diag_id)


def assert_coverage(path, n, z, rad, layout, cfg):
    """Over the matchings of one path and size: which slots carry a QUALIFYING term, from the index maps above.  At n >=
    FULL_COVERAGE_N asserted: every rotation 0 .. 63, every wave, both chains (fused tick), tile shifts 0, 1, 2 and n_t / 2 (fused /
    symmetric); every row k of a wave, every team wave and every lane (ordered kernel).  Returns a line for the log."""
    n_t = (n + 63) // 64
    acc = {k: set() for k in ("sigma", "wave", "chain", "shift", "step", "row", "team", "lane")}
    for m in path_matchings(path, n):
        crowd = isolated_pairs(n, m, SEED + n, z, layout)
        ref = reference(crowd, cfg)
        i = np.nonzero(ref.qualifying)[0]
        j = crowd.partner[i]
        if path.startswith("fused"):
            nw = fused_waves(n, path.endswith("geo"))
            kind, shift, sigma, wave, chain, step = slots_fused(n, i, j, nw)
            off = kind > 0
            acc["sigma"] |= set(sigma[off].tolist())
            acc["wave"] |= set(fused_wave_id(n, i, j, nw).tolist())
            acc["chain"] |= set(chain.tolist())
            acc["step"] |= set(step.tolist())
            acc["shift"] |= set(shift.tolist())
        elif path in ("sym", "list"):
            shift, sigma, wave, step = slots_symmetric(n, i, j)
            acc["sigma"] |= set(sigma[shift > 0].tolist())
            acc["wave"] |= set(wave.tolist())
            acc["step"] |= set(step.tolist())
            acc["shift"] |= set(shift.tolist())
        else:
            _, ipw, team = path.split("-")
            k, w, lane = slots_ordered(i, j, int(ipw), int(team))
            acc["row"] |= set(k.tolist())
            acc["team"] |= set(w.tolist())
            acc["lane"] |= set(lane.tolist())
    if n >= FULL_COVERAGE_N and path != "list":
        if path.startswith("fused") or path == "sym":
            nw = fused_waves(n, path.endswith("geo")) if path.startswith("fused") else 4
            assert acc["sigma"] == set(range(64)), (path, n, sorted(set(range(64)) - acc["sigma"]))
            assert acc["wave"] == set(range(nw)), (path, n, acc["wave"])
            assert acc["step"] == set(range(128 // nw if path.startswith("fused") else 16)), (path, n, acc["step"])
            assert {0, 1, 2, n_t // 2} <= acc["shift"], (path, n, sorted(acc["shift"]))
            if path.startswith("fused"):
                assert acc["chain"] == {0, 1}
        else:
            _, ipw, team = path.split("-")
            assert acc["row"] == set(range(int(ipw))) and acc["team"] == set(range(int(team))) and acc["lane"] == set(range(64)), (path, n)
    return f"{path} N={n}: " + "  ".join(f"{k} {len(v)}" for k, v in acc.items() if v)
