"""A float64 ray cast, and the interval the range scan's fp32 rules (include/sfm_hip.h, ABI 17) must land in.

The reference is written from the geometry.  A row stands at o, a ray leaves it along the unit vector u^ = u / |u| (u the fp32
direction, normalised in float64; in frame 1 turned by the row's heading first), a disc has centre p and radius r (the fp32 value).
The ray meets the disc where |o + s u^ - p|^2 = r^2, that is  s^2 - 2 (a.u^) s + |a|^2 - r^2 = 0  with a = p - o:
    t* = a.u^,   q* = t*^2 - |a|^2 + r^2 (a quarter of the discriminant),   w* = sqrt(q*),   roots t* -+ w*.
No real root (q* < 0): no hit.  Larger root negative: the disc lies wholly behind the origin, no hit.  Smaller root negative and
larger not: the origin is inside, range 0.  Otherwise the range is the smaller root, formed as (|a|^2 - r^2) / (t* + w*) so that it
does not cancel.  Candidates and their order come from the arrays the device is given (``pack_scenes``' state and its three geometry
CSRs): the scene's other pedestrians ascending, then its border, static-obstacle and vehicle points, polylines and points in order.
Frame 1 turns the rays by the float64 heading of the fp32 state, with the header's decision: v if |v| > 0, else the goal entry
(wx - x, wy - y), else (1, 0).

What the rules may give.  eps = 2^-24 bounds the relative error of one correctly rounded fp32 operation.  The rules use a direction
u~ that differs from u^: u~ = n u^ + D with n = |u| and, in frame 0, D = 0.  Write eta = |n - 1| (for an fp32 cos/sin pair
| |u|^2 - 1 | <= 2 eps, so eta <= eps; it is measured per ray, not assumed), d = |a|, c* = the cross product a x u^,
|c*| = sqrt(d^2 - t*^2), and mx, my for the bounds |n u^x| + Dx, |n u^y| + Dy of |u~x|, |u~y|.  Operation by operation:
    ax = RN(px - x), ay = RN(py - y)      each off by at most eps |ax|, eps |ay|               (often exact; paid in full)
    P  = RN(ay uy)                        the rounded product inside the fmaf: another eps |ay| my
    t  = fmaf(ax, ux, P)                  one rounding of the sum: eps (|t*| + what came before)
  so  |t - t*| <= et = Dt + E (1 + eps) + eps (|t*| + Dt),   E = eps |ax| mx + (2 eps + eps^2) |ay| my,
      Dt = eta |t*| + |ax| Dx + |ay| Dy   the price of u~ != u^.
    c  = fmaf(ax, uy, -RN(ay ux))         the same with x and y of the direction exchanged: |c - c*| <= ec.
    r2 = RN(r r)                          formed in double, rounded once: eps r^2
    q  = fmaf(-c, c, r2)                  the product is exact inside the fmaf; c's error enters as ec (2 |c*| + ec); one rounding
  so  |q - q*| <= g = (eps r^2 + ec (2 |c*| + ec)) (1 + eps) + eps |q*|            -- the graze margin g_k.
    w  = RN(sqrt(q))                      sqrt(q* - g) (1 - eps) <= w <= sqrt(q* + g) (1 + eps); away from a graze that is
                                          dw ~ g / 2 w*, at a graze it is sqrt(g): the interval is formed with the square roots
                                          themselves, never with the linearisation
    t + w > 0                             the sign of a rounded sum is the sign of the sum
    s  = RN(t - w)                        eps |s|;  range = max(s, 0)
Frame 1 adds, to D: the heading h~ against the float64 h -- vv = fmaf(vx, vx, RN(vy vy)) is |v|^2 (1 + 2 eps), l = RN(sqrt(vv))
one eps more, the division hx = RN(vx / l) another: each component within kappa = 3 eps of h's; the goal entry pays for
gx = RN(wx - x), gy = RN(wy - y) first, twice (component and length): kappa = 5 eps; (1, 0) is exact -- and the rotation
u~x = fmaf(hx, ux, -RN(hy uy)): Dx = (kappa |hx ux| + (kappa + eps + kappa eps) |hy uy|) (1 + eps) + eps |u'x|, Dy alike, u' the
exactly rotated direction.  The float64 arithmetic of this module is charged too (2^-53 terms: 8 u (d^2 + r^2) on q, 4 u d on t).
Not covered: fp32 underflow and overflow (subnormal products, |v|^2 below 2^-149): ordinary input has none.

Per candidate k that gives [q* - g, q* + g] for q and [t* - et, t* + et] for t, and
    possible   (the rules could call it a hit)   q* + g > 0 and (t* + et) + w_hi > 0
    certain    (the rules must call it a hit)    q* - g > 0 and (t* - et) + w_lo > 0
    lo_k = max(0, (t* - et - w_hi) less eps of itself)      for a possible candidate: t - sqrt(q + g) less the allowance on t
    hi_k = max(0, (t* + et - w_lo) plus eps of itself)      = s_k + e_k: for a certain candidate the allowance e_k on its range
with w_hi = sqrt(max(q* + g, 0)) (1 + eps), w_lo = sqrt(max(q* - g, 0)) (1 - eps).  A possible candidate that is not certain has the
same two bounds (w_lo = 0 then), used only to say which kind a stored range may carry.  Per ray
    lo = min over possible k of lo_k,   hi = min over certain k of hi_k (+inf without one),
    min(lo, Rmax) <= stored range <= min(hi, Rmax);
the stored kind must be that of a possible candidate with lo_k <= range <= hi_k; kind 0 needs range == Rmax and hi >= Rmax.
Every ray is checked: a graze, a tie and a range at Rmax widen the interval, they do not excuse the ray.  How often the interval is
wide is a property of the scenes, counted by ``check`` and bounded by the tests.
"""
import numpy as np

EPS = 2.0 ** -24
U64 = 2.0 ** -53
NEAR_LIMIT = 1.0e15                  # sfm_batch_observe's test of a live row: |x|, |y| below it
KAPPA = {"v": 3.0 * EPS, "goal": 5.0 * EPS, "none": 0.0}


def scene_arrays(pk, b):
    """Scene b of ``pack_scenes``' dict: ({x y vx vy wx wy} fp32 [n], [(px, py) fp32 of borders, static, vehicles])."""
    so = pk["scene_off"]
    st = {k: np.asarray(pk[k][so[b]:so[b + 1]], np.float32) for k in ("x", "y", "vx", "vy", "wx", "wy")}
    geo = []
    for key in ("borders", "static", "dynamic"):
        item_off, off, px, py = pk[key][:4]
        p0, p1 = (int(off[item_off[b]]), int(off[item_off[b + 1]])) if item_off[b + 1] > item_off[b] else (0, 0)
        geo.append((np.asarray(px[p0:p1], np.float32), np.asarray(py[p0:p1], np.float32)))
    return st, geo


def heading64(st, i):
    """The float64 heading of row i from the fp32 state, and which entry gave it."""
    x, y, vx, vy, wx, wy = (np.float64(st[k][i]) for k in ("x", "y", "vx", "vy", "wx", "wy"))
    if np.hypot(vx, vy) > 0:
        l = np.hypot(vx, vy)
        return vx / l, vy / l, "v"
    gx, gy = wx - x, wy - y
    if np.hypot(gx, gy) > 0:
        l = np.hypot(gx, gy)
        return gx / l, gy / l, "goal"
    return 1.0, 0.0, "none"


class Row:
    """One scanned row against all its candidates: kind, order (P,) -- order is the candidate's index in the device's walk, row j at
    j, geometry point g at n + g --; s (the float64 range, +inf where the ray does not meet the disc), lo_k, hi_k (R, P), possible,
    certain (R, P) bool; lo, hi, truth (R,): the interval and the float64 ray cast's own answer before the cap at Rmax."""


def _row(ox, oy, px, py, r, ux, uy, head, Rmax):
    """(ox, oy) float64; px, py, r (P,) float64; ux, uy (R,) the fp32 directions as float64; head None or (hx, hy, source)."""
    n = np.hypot(ux, uy)
    if head is None:
        wx_, wy_ = ux, uy
        Dx = Dy = np.zeros_like(ux)
    else:
        hx, hy, src = head
        k = KAPPA[src]
        wx_, wy_ = hx * ux - hy * uy, hy * ux + hx * uy                # u', the exactly rotated direction: |u'| = n
        Dx = (k * np.abs(hx * ux) + (k + EPS + k * EPS) * np.abs(hy * uy)) * (1 + EPS) + EPS * np.abs(wx_)
        Dy = (k * np.abs(hy * ux) + (k + EPS + k * EPS) * np.abs(hx * uy)) * (1 + EPS) + EPS * np.abs(wy_)
    eta = np.abs(n - 1.0)[:, None]
    hx_, hy_ = (wx_ / n)[:, None], (wy_ / n)[:, None]                  # u^
    mx, my = (np.abs(wx_) + Dx)[:, None], (np.abs(wy_) + Dy)[:, None]
    Dx, Dy = Dx[:, None], Dy[:, None]
    ax, ay = (px - ox)[None, :], (py - oy)[None, :]
    aax, aay = np.abs(ax), np.abs(ay)
    d2 = ax * ax + ay * ay
    r2 = (r * r)[None, :]
    t = ax * hx_ + ay * hy_
    q = t * t - d2 + r2
    cabs = np.sqrt(np.maximum(d2 - t * t, 0.0))
    d = np.sqrt(d2)
    Dt = eta * np.abs(t) + aax * Dx + aay * Dy
    Dc = eta * cabs + aax * Dy + aay * Dx
    Et = EPS * aax * mx + (2 * EPS + EPS * EPS) * aay * my
    Ec = EPS * aax * my + (2 * EPS + EPS * EPS) * aay * mx
    et = Dt + Et * (1 + EPS) + EPS * (np.abs(t) + Dt) + 4 * U64 * d
    ec = Dc + Ec * (1 + EPS) + EPS * (cabs + Dc) + 4 * U64 * d
    g = (EPS * r2 + ec * (2 * cabs + ec)) * (1 + EPS) + EPS * np.abs(q) + 8 * U64 * (d2 + r2)
    w = np.sqrt(np.maximum(q, 0.0))
    w_hi = np.sqrt(np.maximum(q + g, 0.0)) * (1 + EPS)
    w_lo = np.sqrt(np.maximum(q - g, 0.0)) * (1 - EPS)
    o = Row()
    o.possible = (q + g > 0) & (t + et + w_hi > 0)
    o.certain = (q - g > 0) & (t - et + w_lo > 0)
    hit = (q >= 0) & (t + w >= 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(t > 0, (d2 - r2) / (t + w), t - w)                # the smaller root, without cancellation
    o.s = np.where(hit, np.maximum(s, 0.0), np.inf)
    # the bounds, around s where s is well formed (t > 0, a hit), around t - w otherwise
    base = np.where(hit & (t > 0), s, t - w)
    low = base - et - (w_hi - w)
    high = base + et + (w - w_lo)
    o.lo_k = np.where(o.possible, np.maximum(low - EPS * np.abs(low), 0.0), np.inf)
    o.hi_k = np.where(o.possible, np.maximum(high + EPS * np.abs(high), 0.0), np.inf)
    o.lo = o.lo_k.min(axis=1, initial=np.inf)
    o.hi = np.where(o.certain, o.hi_k, np.inf).min(axis=1, initial=np.inf)
    o.truth = o.s.min(axis=1, initial=np.inf)
    return o


def cast(pk, b, directions, max_range, ped_radius, point_radius, frame=0, mask=None):
    """Yields (i, Row) per scanned live row of scene b, ascending.  ``directions`` = (dir_x, dir_y) as the device gets them.
    Candidates that cannot reach the range limit are left out by geometry alone: a ray meets a disc no nearer than d - r, so with
    d - r > 1.001 Rmax + 1e-3 every bound of that candidate lies above Rmax (the allowances are below 1e-5 d), and only
    min(., Rmax) of lo and hi is ever used."""
    st, geo = scene_arrays(pk, b)
    n = len(st["x"])
    ux, uy = (np.asarray(v, np.float32).astype(np.float64) for v in directions)
    Rmax = np.float64(np.float32(max_range))
    rp, rq = np.float64(np.float32(ped_radius)), np.float64(np.float32(point_radius))
    x, y = st["x"].astype(np.float64), st["y"].astype(np.float64)
    gx = np.concatenate([g[0] for g in geo]).astype(np.float64)
    gy = np.concatenate([g[1] for g in geo]).astype(np.float64)
    gkind = np.concatenate([np.full(len(g[0]), 2 + k, np.int64) for k, g in enumerate(geo)])
    allx, ally = np.concatenate([x, gx]), np.concatenate([y, gy])
    allr = np.concatenate([np.full(n, rp), np.full(len(gx), rq)])
    allk = np.concatenate([np.ones(n, np.int64), gkind])
    usable = np.isfinite(allx) & np.isfinite(ally) & (allr > 0)        # (radius 0 switches the kind off; +inf marks an absent ring)
    scanned = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool).reshape(n)
    live = (np.abs(x) < NEAR_LIMIT) & (np.abs(y) < NEAR_LIMIT)
    for i in np.flatnonzero(scanned & live):
        with np.errstate(over="ignore", invalid="ignore"):
            dist = np.hypot(allx - x[i], ally - y[i])
            keep = usable & (dist - allr <= 1.001 * Rmax + 1e-3)
        keep[i] = False
        idx = np.flatnonzero(keep)
        head = heading64(st, i) if frame else None
        o = _row(x[i], y[i], allx[idx], ally[idx], allr[idx], ux, uy, head, Rmax)
        o.kind, o.order, o.Rmax = allk[idx], idx, Rmax
        yield int(i), o


def check(rec, pk, b, directions, max_range, ped_radius, point_radius, frame=0, mask=None, width=None):
    """Holds one scene's record (n, 2R) to the interval.  Returns a dict: ``bad`` (a list of messages, empty when the record is
    inside), ``rays``, ``wide`` (rays whose min(hi, Rmax) - min(lo, Rmax) exceeds ``width``, default 1e-4 max(1, Rmax / 20)),
    ``kinds`` (the stored kinds, 0 the miss, seen on rays that are not wide), ``ratio`` (the worst |range - truth| / allowance, the
    allowance taken on the side of the error), ``at`` (row, ray of that worst), ``first`` (per ray whose nearest candidate is beyond
    doubt, its index in the device's walk: {(row, ray): order})."""
    rec = np.asarray(rec)
    R = len(directions[0])
    Rmax = np.float64(np.float32(max_range))
    width = 1e-4 * max(1.0, Rmax / 20.0) if width is None else width
    out = {"bad": [], "rays": 0, "wide": 0, "kinds": set(), "ratio": 0.0, "at": None, "first": {}}
    n = rec.shape[0]
    seen = np.zeros(n, bool)
    for i, o in cast(pk, b, directions, max_range, ped_radius, point_radius, frame, mask):
        seen[i] = True
        rng, kind = rec[i, :R].astype(np.float64), rec[i, R:]
        lo, hi, truth = np.minimum(o.lo, Rmax), np.minimum(o.hi, Rmax), np.minimum(o.truth, Rmax)
        out["rays"] += R
        wide = hi - lo > width
        out["wide"] += int(wide.sum())
        for ray in range(R):
            if len(o.kind) and o.truth[ray] < Rmax:                     # the nearest beyond doubt: every other bound lies above its own
                j = int(np.argmin(o.s[ray]))
                others = np.delete(o.lo_k[ray], j)
                if o.certain[ray, j] and o.hi_k[ray, j] < Rmax and (others.size == 0 or o.hi_k[ray, j] < others.min()):
                    out["first"][(i, ray)] = int(o.order[j])
            where = f"scene {b} row {i} ray {ray}"
            if not lo[ray] <= rng[ray] <= hi[ray]:
                out["bad"].append(f"{where}: range {rec[i, ray]!r} outside [{lo[ray]!r}, {hi[ray]!r}] (float64 ray cast {truth[ray]!r})")
                continue
            k = int(kind[ray])
            if kind[ray] != k or not 0 <= k <= 4:
                out["bad"].append(f"{where}: kind {kind[ray]!r}")
            elif k == 0:
                if not (rng[ray] == Rmax and o.hi[ray] >= Rmax):
                    out["bad"].append(f"{where}: a miss with range {rec[i, ray]!r}, hi {o.hi[ray]!r}, Rmax {Rmax!r}")
            elif not (rng[ray] < Rmax and ((o.kind == k) & (o.lo_k[ray] <= rng[ray]) & (rng[ray] <= o.hi_k[ray])).any()):
                out["bad"].append(f"{where}: kind {k} at range {rec[i, ray]!r}: no possible candidate of that kind there")
            if not wide[ray]:
                out["kinds"].add(k)
            err = abs(rng[ray] - truth[ray])
            allow = (hi[ray] - truth[ray]) if rng[ray] >= truth[ray] else (truth[ray] - lo[ray])
            if err > 0 and allow > 0 and err / allow > out["ratio"]:
                out["ratio"], out["at"] = err / allow, (i, ray)
    rest = rec[~seen]
    if rest.any():
        out["bad"].append(f"scene {b}: a row that is masked out or not live has a record that is not zero")
    return out


# ---- scenes the host and the GPU tests share ------------------------------------------------------------------------------------

SHIFT = (4096.0, -8192.0)


def _moved(sc, f):
    """A copy of a scene dict with f applied to every (.., 2) coordinate array: rows, goals, borders, rings and centres."""
    sc = dict(sc)
    for k in ("loc", "waypoint"):
        a = np.array(sc[k], dtype=np.float64)
        a[:, :2] = f(a[:, :2])
        sc[k] = a
    sc["borders"] = [f(np.asarray(p, dtype=np.float64)) for p in sc.get("borders", [])]
    if sc.get("border_centers") is not None:
        sc["border_centers"] = f(np.asarray(sc["border_centers"], dtype=np.float64).reshape(-1, 2))
    for k in ("static_obstacles", "dynamic_obstacles"):
        sc[k] = [(f(np.asarray(c, dtype=np.float64).reshape(-1)[:2]), f(np.asarray(r, dtype=np.float64))) for c, r in (sc.get(k) or [])]
    return sc


def shifted(sc, by=SHIFT):
    return _moved(sc, lambda a: a + np.float64(by))


def quantised(sc, step=2.0 ** -10):
    """Every coordinate a multiple of ``step``: shifted by multiples of it, every difference of two coordinates is the same float."""
    return _moved(sc, lambda a: np.round(a / step) * step)


def bare(loc, vel=None, wp=None, borders=(), statics=(), vehicles=()):
    """A scene dict from rows (n, 2) and point lists per kind."""
    loc = np.asarray(loc, dtype=np.float64).reshape(-1, 2)
    n = len(loc)
    z = np.zeros((n, 1))
    pl = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in borders]
    ring = lambda rings: [(np.asarray(r, dtype=np.float64).reshape(-1, 2).mean(axis=0), np.asarray(r, dtype=np.float64).reshape(-1, 2))
                          for r in rings]
    return {"loc": np.hstack([loc, z]),
            "vel": np.hstack([np.zeros((n, 2)) if vel is None else np.asarray(vel, dtype=np.float64).reshape(n, 2), z]),
            "waypoint": np.hstack([loc + 1.0 if wp is None else np.asarray(wp, dtype=np.float64).reshape(n, 2), z]),
            "target_speed": np.ones(n), "borders": pl,
            "border_centers": np.array([p.mean(axis=0) for p in pl]).reshape(-1, 2), "border_lengths": np.ones(len(pl)),
            "static_obstacles": ring(statics), "dynamic_obstacles": ring(vehicles)}
