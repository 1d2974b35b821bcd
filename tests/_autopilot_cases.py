"""Cases and bounds shared by the vehicle-autopilot tests (test_batch_autopilot_host.py, test_batch_autopilot_gpu.py).

The bounds are DERIVED from the roundings of the rule in include/sfm_hip.h (sfm_batch_set_vehicle_autopilot), not tuned; u = 2^-24 is
the unit roundoff of fp32, every fmaf is one rounding, sqrtf and / are correctly rounded.  A star marks the float64 value.

Step 5 against ``autopilot.idm_f64`` from the same fp32 inputs (s, u, gap, settings, dt are exact in both):
    q  = fl(s / v0)                      rel. error u
    q2 = fl(q q)                         rel. 3u            (two factors of 1 + u, one rounding)
    r4 = fl(q2 q2)                       rel. 7u            => |r4 - r4*| <= 7u r4
    g  = max(gap, floor)                 exact
    dv = fl(s - u)                       rel. u
    k2 = 2 fl(sqrt(fl(acc dec)))         rel. 1.5u          (the square root halves the product's u, its own rounding adds u)
    B  = fl(fl(s dv) / k2)               rel. 4.5u          (u of dv, u of the product, 1.5u of k2, u of the quotient)
    dyn = fmaf(s, T, B)                  |error| <= 4.5u |B| + u |dyn|  =: E_dyn   (one rounding of the exact s T + B)
    m  = max(dyn, 0)                     |error| <= E_dyn                           (max is 1-Lipschitz)
    sstar = fl(s0 + m)                   |error| <= E_dyn + u sstar     =: E_ss
    ratio = fl(sstar / g)                rel. E_ss / sstar + u
    inter = fl(ratio ratio)              |error| <= inter (2 E_ss / sstar + 3u)     =: E_int
    w  = fl(1 - r4)                      |error| <= 7u r4 + u |w|
    x  = fl(w - inter)                   |error| <= 7u r4 + u |w| + E_int + u |x|   =: E_x
    araw = fl(acc x)                     |error| <= acc E_x + u |araw|  =: E_a
    a  = max(araw, -brake)               |error| <= E_a                             (1-Lipschitz)
    s' = max(fmaf(dt, a, s), 0)          |error| <= dt E_a + u |s + dt a|           (1-Lipschitz)
``speed_terms`` evaluates this in float64 at the float64 values, times (1 + 1e-3) for the second-order terms.  A max / clamp is
1-Lipschitz, so the bound holds across its switch too; the tests still leave out the draws within the bound of a switch, as the two
sides may differ there in WHICH branch they took, and cap their share.

Free acceleration, no leader: s' = f(s) = s + dt acc (1 - (s / v0)^4).  f is increasing on [0, v0] while 4 dt acc / v0 =: kappa < 1,
and f(v0) = v0, so in exact arithmetic the speed rises and never passes v0.  One tick adds at most eps = u (9 v0 + 10 dt acc): the
step bound above without a leader (r4 <= 1: dt (acc 9u + u acc) + u v0) plus the projection of v' = s' h' back on h' (|h'|^2 - 1 <= 6u,
_driving_cases.H2_BOUND, and two roundings: 8u v0).  Above v0 by e the map contracts, e' <= e (1 - kappa) + eps ((1 + e / v0)^4 - 1
>= 4 e / v0), so the overshoot stays below eps / kappa: ``overshoot_bound``.

Below the standstill gap: for gap <= s0 and s > 0, sstar >= s0 + s T gives inter >= (1 + s T / s0)^2 >= 1 + 2 s T / s0, so
a <= -mu s with mu = 2 acc T / s0 (while mu s <= brake, which the cases keep).  From the first tick at or below s0, entered at speed
s_e, the speed decays by (1 - mu dt) per tick and the vehicle travels at most dt s_e / (mu dt); the entering tick itself adds dt
s_e.  So the gap never falls below s0 - s_e (dt + 1 / mu): ``undershoot_bound``, plus ``POSITION_SLACK`` for the roundings of the
positions (T u max|c| for T ticks, as in _driving_cases.centre_bound).
"""
import numpy as np

import _driving_cases as D
from carla_social_force_model_amd import autopilot as A
from carla_social_force_model_amd import scenarios

U = 2.0 ** -24
POSITION_SLACK = 400 * U * 200.0 * (1.0 + 1e-3)          # 400 ticks, |coordinate| <= 200 m


def speed_terms(s, u, gap, led, st, dt):
    """The float64 intermediates of step 5 the bound and the switch tests need: (dyn, araw, s + dt a, the bound on |s' - s'*|, the
    bound on |araw - araw*|, the bound on |dyn - dyn*|)."""
    s, u, gap, dt = (np.float64(np.float32(x)) for x in (s, u, gap, dt))
    v0, T, s0, acc, dec, brake = (np.float64(np.float32(x)) for x in st[:6])
    r4 = (s / v0) ** 4
    dyn, inter, e_int, e_dyn = 0.0, 0.0, 0.0, 0.0
    if led:
        g = max(gap, np.float64(A.GAP_FLOOR))
        B = s * (s - u) / (2.0 * np.sqrt(acc * dec))
        dyn = s * T + B
        e_dyn = 4.5 * U * abs(B) + U * abs(dyn)
        sstar = s0 + max(dyn, 0.0)
        e_ss = e_dyn + U * sstar
        inter = (sstar / g) ** 2
        e_int = inter * (2.0 * e_ss / sstar + 3.0 * U)
    w = 1.0 - r4
    x = w - inter
    e_x = 7.0 * U * r4 + U * abs(w) + e_int + U * abs(x)
    araw = acc * x
    e_a = acc * e_x + U * abs(araw)
    a = max(araw, -brake)
    sn = s + dt * a
    return dyn, araw, sn, (dt * e_a + U * abs(sn)) * (1.0 + 1e-3), e_a * (1.0 + 1e-3), e_dyn * (1.0 + 1e-3)


def near_a_switch(s, u, gap, led, st, dt):
    """Is the draw within the derived bound of a max / clamp switch of step 5 (dyn = 0, araw = -brake, s + dt a = 0)?"""
    dyn, araw, sn, e_s, e_a, e_dyn = speed_terms(s, u, gap, led, st, dt)
    brake = np.float64(np.float32(st[5]))
    return bool((led and abs(dyn) < e_dyn) or abs(araw + brake) < e_a or abs(sn) < e_s)      # (strict: exact on both sides is no switch)


def overshoot_bound(st, dt):
    v0, acc = float(st[0]), float(st[3])
    kappa = 4.0 * dt * acc / v0
    assert kappa < 1.0
    return U * (9.0 * v0 + 10.0 * dt * acc) * (1.0 + 1e-3) / kappa


def undershoot_bound(s_e, st, dt):
    T, s0, acc, brake = float(st[1]), float(st[2]), float(st[3]), float(st[5])
    mu = 2.0 * acc * T / s0
    assert mu * dt < 1.0 and mu * s_e <= brake
    return s_e * (dt + 1.0 / mu) + POSITION_SLACK


def street(vehicles, peds=(), ped_vel=None):
    """A scene dict without borders: ``vehicles`` a list of (centre, yaw, velocity), ``peds`` (N, 2) positions."""
    ext = (2.4, 1.0)
    local = scenarios.ring_local_offsets(*ext)
    peds = np.asarray(peds, dtype=np.float64).reshape(-1, 2)
    n = len(peds)
    pv = np.zeros((n, 2)) if ped_vel is None else np.asarray(ped_vel, dtype=np.float64).reshape(n, 2)
    f = lambda a: np.float32(a).astype(np.float64)
    sc = {"loc": f(np.column_stack((peds, np.zeros(n)))), "vel": f(np.column_stack((pv, np.zeros(n)))),
          "waypoint": f(np.column_stack((peds + 50.0 * pv, np.zeros(n)))), "target_speed": f(np.linalg.norm(pv, axis=1) if n else np.zeros(0)),
          "radius": np.full(n, 0.3), "mode": np.zeros(n, int), "borders": [], "border_centers": np.zeros((0, 2)),
          "border_lengths": np.zeros(0), "static_obstacles": [],
          "dynamic_obstacles": [(f(c), scenarios.place_ring_f32(f(c), yaw, local)) for c, yaw, _ in vehicles],
          "dynamic_vel": f(np.array([v for _, _, v in vehicles], dtype=np.float64).reshape(-1, 2)),
          "dynamic_yaw": np.array([yaw for _, yaw, _ in vehicles], dtype=np.float64),
          "dynamic_extent": np.array([ext] * len(vehicles), dtype=np.float64).reshape(-1, 2)}
    sc["dynamic_heading"] = scenarios.vehicle_headings(sc)
    return sc


def peds_of(sc):
    loc, vel = np.asarray(sc["loc"], dtype=np.float64), np.asarray(sc["vel"], dtype=np.float64)
    return np.column_stack((loc[:, :2], vel[:, :2])) if len(loc) else np.zeros((0, 4))


def run_twin(sc, paths, st, fl, dt, ticks, move_peds=None, commands=None):
    """``ticks`` controller launches of the twin, each followed by the move (``scenarios.drive_vehicles``); ``move_peds(sc, t)``
    moves the pedestrians by hand.  Returns the records (ticks, M, 8), the cursors (ticks, M) and the centres (ticks + 1, M, 2)."""
    M = len(sc["dynamic_obstacles"])
    cur = np.zeros(M, np.int32)
    cmd = commands
    recs, curs, ctrs = [], [], [np.array([c for c, _ in sc["dynamic_obstacles"]])]
    for t in range(ticks):
        cmd, cur, rec = A.autopilot_scene(sc, peds_of(sc), paths, st, fl, cur, dt, cmd)
        scenarios.drive_vehicles(sc, cmd[:, 3], cmd[:, :3], dt)
        if move_peds is not None:
            move_peds(sc, t)
        recs.append(rec)
        curs.append(cur.copy())
        ctrs.append(np.array([c for c, _ in sc["dynamic_obstacles"]]))
    return np.array(recs), np.array(curs), np.array(ctrs)


# the settings of the behaviour cases: over-damped about the standstill gap (omega T / 2 = sqrt(2 acc / s0) T / 2 = 1.06 >= 1), so
# the float64 restatement itself comes to rest above s0; mu = 2 acc T / s0 = 3 /s, mu v0 <= brake
# (the roots of lambda^2 + omega^2 T lambda + omega^2, omega^2 = 2 acc / s0 = 2, are -1 /s and -2 /s: the approach to the standstill
# gap decays as e^-t, and "stopped" below means a speed under STOPPED v0 = e^-6 v0 once the last 6 s were spent on it)
STOPPED = float(np.exp(-6.0))
CALM = dict(v0=3.0, T=1.5, s0=2.0, acc=2.0, dec=2.0, brake=9.0, half_width=1.2, front=2.5, look=40.0, reach=3.0, ped_margin=0.5,
            max_turn=0.06)


def standing_pedestrian(ahead=30.0):
    """One vehicle at the origin heading +x at rest, a pedestrian standing in its lane ``ahead`` m ahead, a path point far beyond."""
    sc = street([((0.0, 0.0), 0.0, (0.0, 0.0))], peds=[(ahead, 0.25)])
    return sc, [[np.array([[200.0, 0.0]])]]


def closed_path():
    """One vehicle on a closed path of 8 points (a regular octagon of radius 12 m), starting on it heading along it."""
    ang = 2.0 * np.pi * np.arange(8) / 8.0
    pts = 12.0 * np.column_stack((np.cos(ang), np.sin(ang)))
    sc = street([((12.0, -3.0), np.pi / 2.0, (0.0, 0.0))])
    return sc, [[pts]]


def draws(n, seed):
    """n random (s, u, gap, led, settings row, dt) of step 5: speeds up to 1.2 v0, leaders of both relative speeds, gaps from inside
    the floor to far, a fifth without a leader."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        acc = rng.uniform(0.5, 3.0)
        dec = rng.uniform(0.5, 4.0)
        kw = dict(v0=rng.uniform(2.0, 20.0), T=rng.uniform(0.0, 2.5), s0=rng.uniform(0.5, 4.0), acc=acc, dec=dec,
                  brake=dec + rng.uniform(0.0, 6.0))
        st = np.zeros(A.N_SETTINGS, np.float32)
        st[:6] = [kw[k] for k in A.SETTINGS[:6]]
        s = np.float32(rng.uniform(0.0, 1.2) * kw["v0"]) if rng.random() > 0.1 else np.float32(0.0)
        u = np.float32(rng.uniform(-2.0, 1.5 * kw["v0"]))
        gap = np.float32(np.exp(rng.uniform(np.log(0.005), np.log(80.0))) if rng.random() > 0.05 else rng.uniform(-1.0, 0.01))
        out.append((s, u, gap, rng.random() > 0.2, st, np.float32(rng.choice([0.02, 0.04, 0.05, 0.1]))))
    return out


# ---- the mixed batch of the device tests --------------------------------------------------------------------------------------

def path_near(rng, sc, k, points):
    c = np.asarray(sc["dynamic_obstacles"][k][0], dtype=np.float64)
    if not np.isfinite(c).all():
        c = np.array([5.0, 5.0])
    yaw = float(sc["dynamic_yaw"][k])
    ahead = np.cumsum(rng.uniform(1.0, 4.0, points))
    side = rng.uniform(-2.5, 2.5, points)
    return c + np.column_stack((ahead * np.cos(yaw) - side * np.sin(yaw), ahead * np.sin(yaw) + side * np.cos(yaw)))
