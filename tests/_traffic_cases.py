"""Seeded inputs of the gap-acceptance and vehicle-ring fixtures (tests/golden/traffic/*.npz).  NumPy only.

The fixtures do not store inputs: tests/golden/make_golden_traffic.py and the tests both build them here, and a fixture records the
SHA-256 of what it was written for (``digest``), so an edit of this file shows up as a failed drift guard, not as a silent
change of what is tested.  Every value is float32-representable, so the reference's float64 and the device's fp32 start from
identical numbers.

A case set is a dict of arrays.  Cases come in GROUPS that share one vehicle set (a batch scene, a handle's crowd):
``group_off`` [G+1] cases of group g, ``veh_off`` [G+1] its vehicles in ``veh_loc`` / ``veh_vel`` / ``veh_ext`` (M,2);
per case ``loc``, ``goal`` (C,2), ``speed``, ``margin`` (C,) and ``kind`` (C,) -- an index into ``KINDS``.

Decision slack (oracle.sfm_oracle.gap_slack): a random case is DECIDED when its slack is at least ``SLACK_BAND``.  Where the band
comes from: fp32 rounds the end points of the two paths at the magnitude of the coordinates -- up to ~150 m here, half an ulp
4e-6 m, a few roundings each, so ~1e-5 m -- against path lengths of a metre or more: ~1e-5 on t and u where the paths
cross squarely, and 1 / sin(angle) times that where they do not, which is why gap_slack multiplies by the sine.  Times to the
meeting point inherit the same ~1e-5 relative.  1e-4 (the band the device-mode tests already use for borderline arrivals) is ten
times that estimate.  At most ``UNDECIDED_CAP`` of the random class may fall inside the band.  The exact class has no band."""
import hashlib

import numpy as np

SLACK_BAND = 1e-4
UNDECIDED_CAP = 0.01
ROBUST_SLACK = 1e-2          # the hand-built cases that are not exact in fp32 (diagonal headings) sit at least this far from a boundary
RESOLUTION = 0.1

KINDS = ("random", "touch_t0", "touch_t1", "touch_u0", "touch_u1", "touch_t1_u1", "parallel_distinct", "collinear_overlap",
         "collinear_head_on", "collinear_one_point", "collinear_disjoint", "stationary_on_path", "stationary_then_refusing",
         "tie_front", "next_to_tie_front", "tie_back", "next_to_tie_back", "first_extent_decides", "diagonal_extent_product",
         "standing_on_path", "standing_off_path", "standing_past_the_end", "standing_on_parked_vehicle", "plain_crossing")
EXACT_KINDS = tuple(k for k in KINDS[1:] if k not in ("diagonal_extent_product",) and not k.startswith("standing"))
DEGENERATE_KINDS = tuple(k for k in KINDS if k.startswith("standing"))


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def digest(arrays):
    """SHA-256 over the named arrays' dtype, shape and bytes, in key order."""
    h = hashlib.sha256()
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h.update(f"{k}:{a.dtype.str}:{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _assemble(groups):
    """groups: list of (veh_loc (m,2), veh_vel (m,2), veh_ext (m,2), loc (n,2), goal (n,2), speed (n,), margin (n,), kind (n,))."""
    cat = lambda i, w: np.concatenate([np.asarray(g[i], dtype=np.float64).reshape((-1, w) if w else (-1,)) for g in groups])
    out = dict(group_off=np.cumsum([0] + [len(g[5]) for g in groups]).astype(np.int64),
               veh_off=np.cumsum([0] + [len(g[0]) for g in groups]).astype(np.int64),
               veh_loc=cat(0, 2), veh_vel=cat(1, 2), veh_ext=cat(2, 2), loc=cat(3, 2), goal=cat(4, 2), speed=cat(5, 0),
               margin=cat(6, 0), kind=cat(7, 0).astype(np.int16))
    for k, a in out.items():
        if a.dtype == np.float64:
            assert np.array_equal(a, f32(a)), f"{k} is not float32-representable"
    return out


def group(cs, g):
    """Vehicle set and case slice of group g: (veh_loc, veh_vel, veh_ext, slice)."""
    v = slice(int(cs["veh_off"][g]), int(cs["veh_off"][g + 1]))
    return cs["veh_loc"][v], cs["veh_vel"][v], cs["veh_ext"][v], slice(int(cs["group_off"][g]), int(cs["group_off"][g + 1]))


def group_of_case(cs):
    return np.repeat(np.arange(len(cs["group_off"]) - 1), np.diff(cs["group_off"]))


def vehicle_yaw(vel):
    """Heading of a vehicle set for the device's oriented boxes (rings only; gap acceptance does not read it)."""
    return np.arctan2(vel[:, 1], vel[:, 0])


def describe(cs, i):
    g = int(group_of_case(cs)[i])
    vl, vv, ve, _ = group(cs, g)
    return (f"case {i} ({KINDS[cs['kind'][i]]}, group {g}): loc {cs['loc'][i].tolist()} goal {cs['goal'][i].tolist()} speed "
            f"{cs['speed'][i]!r} margin {cs['margin'][i]!r}; vehicles at {vl.tolist()} moving {vv.tolist()}, extents {ve.tolist()}")


# ------------------------------------------------------------------------------------------------------------------------
# random class
# ------------------------------------------------------------------------------------------------------------------------
RANDOM_SIZES = (4200, 1024) + (100,) * 148          # one group above 4096 (where a handle changes its stepping path), one a full batch scene


def random_cases(seed=20261016, sizes=RANDOM_SIZES):
    """The generator of test_host_logic.py's restatement test without the grid snap, turned round so that many pedestrians share a
    vehicle set: 1-4 vehicles per group (10 % at rest), 70 % of the pedestrians aimed through a point of a vehicle's future path
    so that they get there within +-2 s of the vehicle, margins from {-1, 0, 0.5, 1.5}."""
    rng = np.random.default_rng(seed)
    groups = []
    for n in sizes:
        m = int(rng.integers(1, 5))
        vloc = f32(rng.uniform(-30, 30, (m, 2)))
        h, sp = rng.uniform(0, 2 * np.pi, m), rng.uniform(2, 12, m)
        vvel = f32(np.column_stack((np.cos(h), np.sin(h))) * (sp * (rng.random(m) > 0.1))[:, None])
        ext = f32(rng.uniform(0.5, 2.5, (m, 2)))
        speed = f32(rng.uniform(0.8, 2.0, n))
        margin = rng.choice([-1.0, 0.0, 0.5, 1.5], n)
        k = rng.integers(0, m, n)
        tau = rng.uniform(0, 8, n)
        X = vloc[k] + vvel[k] * tau[:, None]
        a = rng.uniform(0, 2 * np.pi, n)
        d = np.column_stack((np.cos(a), np.sin(a)))
        before = speed * np.maximum(0.25, tau + rng.uniform(-2, 2, n))
        loc, goal = X - d * before[:, None], X + d * rng.uniform(0.5, 10, n)[:, None]
        free = rng.random(n) >= 0.7
        loc[free], goal[free] = rng.uniform(-10, 10, (int(free.sum()), 2)), rng.uniform(-10, 10, (int(free.sum()), 2))
        loc, goal = f32(loc), f32(goal)
        short = np.linalg.norm(goal - loc, axis=1) < 0.5
        goal[short] = f32(loc[short] + 1.0)
        groups.append((vloc, vvel, ext, loc, goal, speed, margin, np.zeros(n)))
    return _assemble(groups)


# ------------------------------------------------------------------------------------------------------------------------
# exact and degenerate classes: hand-built in a canonical frame, then moved around by symmetries that keep fp32 exact
# ------------------------------------------------------------------------------------------------------------------------
def _base_cases():
    """(kind, loc, goal, speed, margin, [(centre, velocity, extent), ...]) in the canonical frame: the pedestrian walks from (0,0)
    along +x; most vehicles drive along +y at 4 m/s with extent (3, 1) -- x-extent and y-extent differ, so reading the wrong
    component moves the front and the back by 2 m."""
    up = lambda x, cy, ext=(3.0, 1.0): ((x, cy), (0.0, 4.0), ext)
    along = lambda cx, vx=4.0, y=0.0: ((cx, y), (vx, 0.0), (3.0, 1.0))
    P = ((0.0, 0.0), (8.0, 0.0), 2.0)                                   # time_ped = 4 s
    far = ((-40.0, 24.0), (4.0, 0.0), (3.0, 4.0))                       # drives away on a parallel line 24 m off: never met
    B = [
        ("plain_crossing", *P, 0.5, [up(4.0, -8.0)]),                   # front 7 m away: 1.75 - 0.5 < 2 < 2.25 + 0.5: refuse
        ("plain_crossing", *P, 0.5, [up(4.0, -24.0)]),                  # path ends before the pedestrian's: accept
        ("plain_crossing", *P, 0.0, [up(2.0, -2.0)]),                   # tti_ped 1: 0.25 < 1 < 0.75 fails: accept
        ("touch_t0", *P, 0.5, [up(0.0, -2.0)]),                         # path through the pedestrian's start: refuse
        ("touch_t0", *P, 0.5, [up(0.0, -8.0)]),                         # ... front 7 m away: accept
        ("touch_t1", *P, 0.5, [up(8.0, -15.0)]),                        # path through the waypoint: 3 < 4 < 4.5: refuse
        ("touch_t1", *P, 0.0, [up(8.0, -16.0)]),                        # ... 3.75 < 4 < 4.25: refuse
        ("touch_u0", *P, 0.5, [up(4.0, 1.0)]),                          # the back stands on the pedestrian's path: accept
        ("touch_u0", *P, 0.5, [up(0.5, 1.0)]),                          # ... pedestrian there within the margin: refuse
        ("touch_u1", *P, 0.5, [up(4.0, -19.0)]),                        # path ENDS on the pedestrian's path: accept
        ("touch_t1_u1", *P, 0.5, [up(8.0, -19.0)]),                     # ... at the waypoint, tti_ped == tti_front - margin: accept
        ("parallel_distinct", *P, 0.5, [along(-4.0, y=2.0)]),
        ("collinear_overlap", *P, 0.5, [along(-10.0)]),                 # from behind, front 7 m off: accept
        ("collinear_overlap", *P, 0.5, [along(-4.0)]),                  # from behind, front 1 m off: refuse
        ("collinear_head_on", *P, 0.5, [along(20.0, -4.0)]),
        ("collinear_one_point", *P, 0.5, [along(-21.0)]),               # path ends on the pedestrian's start: accept
        ("collinear_one_point", *P, 0.5, [along(11.0)]),                # back on the waypoint, driving away: accept
        ("collinear_one_point", (0.0, 0.0), (1.0, 0.0), 2.0, 1.5, [along(4.0)]),          # ... within the margin: refuse
        ("collinear_disjoint", *P, 0.5, [along(20.0)]),
        ("stationary_on_path", *P, 0.5, [((4.0, 0.0), (0.0, 0.0), (3.0, 1.0))]),
        ("stationary_then_refusing", *P, 0.5, [((4.0, 0.0), (0.0, 0.0), (3.0, 1.0)), up(4.0, -8.0)]),
        ("tie_front", *P, 0.5, [up(4.0, -11.0)]),                       # tti_front - margin == tti_ped == 2: accept
        ("next_to_tie_front", *P, 0.5, [up(4.0, -10.5)]),               # 1.875 < 2: refuse
        ("tie_back", *P, 0.5, [up(4.0, -5.0)]),                         # tti_back + margin == tti_ped == 2: accept
        ("next_to_tie_back", *P, 0.5, [up(4.0, -5.5)]),                 # 2.125 > 2: refuse
        ("first_extent_decides", *P, 0.0, [far, up(4.0, -10.0)]),       # first extent y = 4: 1.5 < 2 < 3.5 refuse; its own y = 1: accept
        ("first_extent_decides", *P, 0.0, [((-40.0, 24.0), (4.0, 0.0), (3.0, 0.5)), up(4.0, -6.0, (3.0, 4.0))]),   # the other way round
        ("diagonal_extent_product", *P, 0.5, [((-2.0, -8.0), (3.0, 4.0), (3.0, 0.5))]),
        ("diagonal_extent_product", *P, 0.0, [((1.0, -4.0), (3.0, 4.0), (0.5, 3.0))]),
        ("standing_on_path", (4.0, 0.0), (4.0, 0.0), 2.0, 0.5, [up(4.0, -2.0)]),          # refuse
        ("standing_on_path", (4.0, 0.0), (4.0, 0.0), 2.0, 0.5, [up(4.0, -3.0)]),          # front reaches the spot at the end: tie, accept
        ("standing_off_path", (5.0, 0.0), (5.0, 0.0), 2.0, 0.5, [up(4.0, -2.0)]),         # beside the path: accept
        ("standing_past_the_end", (4.0, 2.0), (4.0, 2.0), 2.0, 0.5, [up(4.0, -2.0)]),     # on its line, beyond its end: accept
        ("standing_on_parked_vehicle", (4.0, 0.0), (4.0, 0.0), 2.0, 0.5, [((4.0, 0.0), (0.0, 0.0), (3.0, 1.0))]),
    ]
    return B


_OPS = [np.array(m, dtype=np.float64) for m in ([[1, 0], [0, 1]], [[0, -1], [1, 0]], [[-1, 0], [0, -1]], [[0, 1], [-1, 0]],
                                                [[-1, 0], [0, 1]], [[1, 0], [0, -1]], [[0, 1], [1, 0]], [[0, -1], [-1, 0]])]
_PLACEMENTS = [(1.0, (0.0, 0.0)), (0.5, (16.0, -32.0)), (2.0, (-3.0, 64.0))]      # (scale, shift): powers of two and small integers


def exact_cases():
    """Every base case under the 8 symmetries of the square (a quarter turn swaps the roles of x- and y-extent, so the extents are
    swapped with it) at three placements; lengths, velocities, extents and the pedestrian's speed scale together, so times do not."""
    groups = []
    for kind, loc, goal, speed, margin, vehicles in _base_cases():
        for op in _OPS:
            swap = op[0, 0] == 0
            for scale, shift in _PLACEMENTS:
                mv = lambda p: (op @ np.asarray(p, dtype=np.float64)) * scale + np.asarray(shift)
                vl = np.array([mv(c) for c, _, _ in vehicles])
                vv = np.array([(op @ np.asarray(v)) * scale for _, v, _ in vehicles])
                ve = np.array([(e[::-1] if swap else e) for _, _, e in vehicles], dtype=np.float64) * scale
                groups.append((vl, vv, ve, mv(loc)[None], mv(goal)[None], [speed * scale], [margin], [KINDS.index(kind)]))
    return _assemble(groups)


def closed_form(loc, goal, speed, margin, vloc, vvel, ext0, dtype):
    """The fp32 closed form of the device (sfm_interaction.h gap_accepted) in NumPy scalars of ``dtype``, without fused
    multiply-adds.  Returns (accepted, operands): every comparison it took as (name, lhs, rhs).  Used twice by
    ``assert_exact``: where all intermediates are exact, float32 and float64 give the same operands bit for bit."""
    T = dtype
    loc, goal, ext0 = np.asarray(loc, T), np.asarray(goal, T), np.asarray(ext0, T)
    speed, margin = T(speed), T(margin)
    ops = []

    def cmp(name, a, b):
        ops.append((name, float(a), float(b)))

    def seg_dist(a, b, p):
        ab = b - a
        ab2 = ab[0] * ab[0] + ab[1] * ab[1]
        t = ((p[0] - a[0]) * ab[0] + (p[1] - a[1]) * ab[1]) / ab2 if ab2 > 0 else T(0)
        t = min(max(t, T(0)), T(1))
        q = a + t * ab - p
        return np.sqrt(q[0] * q[0] + q[1] * q[1])

    if margin < 0:
        return True, ops
    r = goal - loc
    rr = r[0] * r[0] + r[1] * r[1]
    time_ped = np.sqrt(rr) / speed
    for c, v in zip(np.asarray(vloc, T), np.asarray(vvel, T)):
        sp = np.sqrt(v[0] * v[0] + v[1] * v[1])
        inv = T(1) if sp == 0 else T(1) / sp
        o = v * inv * ext0
        front, back = c + o, c - o
        vgoal = front + v * (time_ped + margin)
        s, qp = vgoal - back, back - loc
        rxs, qpxr = r[0] * s[1] - r[1] * s[0], qp[0] * r[1] - qp[1] * r[0]
        cmp("rxs != 0", rxs, 0.0)
        hit, h0, h1 = False, None, None
        if rxs != 0:
            t, u = (qp[0] * s[1] - qp[1] * s[0]) / rxs, qpxr / rxs
            for name, a, b in (("t >= 0", t, 0.0), ("t <= 1", t, 1.0), ("u >= 0", u, 0.0), ("u <= 1", u, 1.0)):
                cmp(name, a, b)
            if 0 <= t <= 1 and 0 <= u <= 1:
                hit, h0 = True, loc + t * r
                h1 = h0
        elif rr > 0:
            cmp("qpxr == 0", qpxr, 0.0)
            if qpxr == 0:
                t0 = (qp[0] * r[0] + qp[1] * r[1]) / rr
                t1 = t0 + (s[0] * r[0] + s[1] * r[1]) / rr
                lo, hi = max(T(0), min(t0, t1)), min(T(1), max(t0, t1))
                cmp("lo <= hi", lo, hi)
                if lo <= hi:
                    hit, h0, h1 = True, loc + lo * r, loc + hi * r
        else:
            ss, w = s[0] * s[0] + s[1] * s[1], -(qp[0] * s[0] + qp[1] * s[1])
            if ss > 0:
                cmp("on the line", qp[0] * s[1] - qp[1] * s[0], 0.0)
                cmp("w >= 0", w, 0.0)
                cmp("w <= ss", w, ss)
                hit = bool(qp[0] * s[1] - qp[1] * s[0] == 0 and 0 <= w <= ss)
            else:
                hit = bool(qp[0] == 0 and qp[1] == 0)
            h0 = h1 = loc
        if not hit or sp == 0:
            continue
        tti_ped = seg_dist(h0, h1, loc) / speed
        tti_front, tti_back = seg_dist(h0, h1, front) / sp, seg_dist(h0, h1, back) / sp
        cmp("tti_front - margin < tti_ped", tti_front - margin, tti_ped)
        cmp("tti_ped < tti_back + margin", tti_ped, tti_back + margin)
        if tti_front - margin < tti_ped < tti_back + margin:
            return False, ops
    return True, ops


def assert_exact(cs, i, far=1e-3):
    """The exactness claim of one hand-built case: evaluated in float32 and in float64, the closed form takes the same
    comparisons, and the operands of each either agree bit for bit (float64 carries 29 more bits: agreement means the fp32 value is
    the exact one) or sit at least ``far`` (relative) from their boundary in both.  Returns the decision."""
    vl, vv, ve, _ = group(cs, int(group_of_case(cs)[i]))
    args = (cs["loc"][i], cs["goal"][i], cs["speed"][i], cs["margin"][i], vl, vv, ve[0])
    d32, o32 = closed_form(*args, np.float32)
    d64, o64 = closed_form(*args, np.float64)
    assert d32 == d64 and [o[0] for o in o32] == [o[0] for o in o64], describe(cs, i)
    for (name, a, b), (_, a64, b64) in zip(o32, o64):
        same = a == a64 and b == b64
        gap = min(abs(a - b), abs(a64 - b64)) / max(1.0, abs(a64), abs(b64))
        assert same or gap >= far, f"{describe(cs, i)}: {name} is neither exact nor far: fp32 {a!r} vs {b!r}, float64 {a64!r} vs {b64!r}"
    return d32


# ------------------------------------------------------------------------------------------------------------------------
# vehicle rings
# ------------------------------------------------------------------------------------------------------------------------
def ring_cases(seed=20261017, n_random=110):
    """Two sets of vehicles, each (centre (V,2), yaw (V,) radians, extent (V,2)).  ``random``: centres to +-500 m, any yaw, extents
    0.3-3.0 x 0.3-1.5.  ``edge``: for 20 point counts n, three extents whose circumference 2 ex + 2 ey is n / 10 to within one fp32 ulp of ey, from
    below, nearest and from above -- ``int(circumference / 0.1)`` truncates, so the point COUNT is the edge: n - 1 or n -- and six
    extents small enough for the ``max(6, ...)`` floor."""
    rng = np.random.default_rng(seed)
    rnd = (f32(rng.uniform(-500, 500, (n_random, 2))), f32(rng.uniform(0, 2 * np.pi, n_random)),
           f32(np.column_stack((rng.uniform(0.3, 3.0, n_random), rng.uniform(0.3, 1.5, n_random)))))
    keep = []
    for n in rng.choice(np.arange(13, 88), 20, replace=False):            # 2 ex + 2 ey = n / 10 up to fp32 rounding, from both sides
        ex = np.float32(rng.uniform(0.3, min(3.0, n / 20.0 - 0.3)))
        ey = np.float32((n * RESOLUTION - 2.0 * np.float64(ex)) / 2.0)
        keep += [(ex, np.nextafter(ey, np.float32(-np.inf))), (ex, ey), (ex, np.nextafter(ey, np.float32(np.inf)))]
    keep += [(0.125, 0.125), (0.125, 0.25), (0.0625, 0.125), (0.15625, 0.125), (0.1875, 0.125), (0.140625, 0.15625)]   # 4, 7, 3, 5, 6, 5 -> floor at 6
    ext = f32(np.array(keep))
    edge = (f32(rng.uniform(-500, 500, (len(keep), 2))), f32(rng.uniform(0, 2 * np.pi, len(keep))), ext)
    return {"random": rnd, "edge": edge}


def ring_inputs(v):
    return dict(center=v[0], yaw=v[1], extent=v[2])
