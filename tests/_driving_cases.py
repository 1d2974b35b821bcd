"""Cases and bounds shared by the driven-vehicle tests (test_batch_driving_host.py, test_batch_driving_gpu.py).

The bounds are DERIVED from the roundings of the rule in include/sfm_hip.h (drive_vehicle), not tuned; u = 2^-24 is the unit
roundoff of fp32, every fmaf is one rounding, sqrtf and / are correctly rounded.

|h|^2 - 1 after ONE normalisation (kind 2; it does not depend on the heading that came in, so nothing accumulates):
    n2 = fmaf(gx, gx, fl(gy gy)) = |g|^2 (1 + e),  |e| <= 2u + u^2        (the product, then the fused sum)
    n  = fl(sqrt(n2))            = |g| sqrt(1 + e) (1 + d3),              |d3| <= u
    h' = (fl(gx / n), fl(gy / n)):  |h'|^2 = (|g| / n)^2 (1 + d)^2,       |d| <= u
    => | |h'|^2 - 1 | <= |e| + 2 |d3| + 2 |d| + O(u^2) = 6u + O(u^2).     H2_BOUND = 6u + 64 u^2.

The centre against the same semi-implicit scheme in float64 (turn, normalise, v = a h', c += dt v, from the same fp32 inputs):
  direction of the heading.  The float64 map g = [[b, -c], [c, b]] h is a similarity, so it carries an angular error through
    unchanged, and the normalisation changes no direction.  What one fp32 tick adds: gx = fmaf(b, hx, -fl(c hy)) is off by at most
    u |c hy| + u |gx| <= 2u (1 + 8u) (|h| <= 1 + 3u, |(b, c)| <= 1 + u), likewise gy: a vector error <= 2 sqrt(2) u on |g| ~ 1;
    the two divisions add a relative u per component, a vector error <= u.  Per tick E_H = (2 sqrt(2) + 1) u, after t ticks t E_H.
  length of the heading: | |h'| - 1 | <= 3u + O(u^2) (half of the above).
  velocity v' = fl(a h'): off the float64 a h by at most |a| (t E_H + 3u + u).
  centre c' = fmaf(dt, v', c): the step carries dt times the velocity error, the one rounding adds u |c'|.
  => after T ticks  |c - c64| <= sum_t dt |a_t| ((t + 1) E_H + 4u) + T u max|c|,  times (1 + 1e-3) for the second-order terms.
"""
import numpy as np

from carla_social_force_model_amd import scenarios

U = 2.0 ** -24
H2_BOUND = 6.0 * U + 64.0 * U * U
E_H = (2.0 * np.sqrt(2.0) + 1.0) * U


def centre_bound(dt, speeds, cmax):
    """The bound above for a run of len(speeds) ticks: per-tick signed speeds a_t, step dt, cmax >= every |coordinate| on the way."""
    a = np.abs(np.asarray(speeds, dtype=np.float64))
    t = np.arange(1, len(a) + 1, dtype=np.float64)
    return (float(np.sum(dt * a * (t * E_H + 4.0 * U))) + len(a) * U * float(cmax)) * (1.0 + 1e-3)


def turn_commands(T, seed, max_speed=5.0, max_turn=0.04):
    """T unicycle commands (a, cos dpsi, sin dpsi) float32: speeds of both signs (a quarter of the run reverses), turns of both
    signs, the cos / sin taken in float64 and rounded once."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.5, max_speed, T) * np.where((np.arange(T) // (T // 8 or 1)) % 4 == 3, -1.0, 1.0)
    dpsi = rng.uniform(-max_turn, max_turn, T) + max_turn * 0.5 * np.sin(np.arange(T) * 0.01)
    return np.column_stack((a, np.cos(dpsi), np.sin(dpsi))).astype(np.float32)


def unicycle64(c0, h0, cmds, dt):
    """The same semi-implicit scheme in float64, from the same fp32 inputs: per tick g = R(b, c) h, h' = g / |g|, v' = a h',
    c' = c + dt v'.  Returns the centres (T + 1, 2) and headings (T + 1, 2)."""
    c, h = np.asarray(c0, dtype=np.float64).copy(), np.asarray(h0, dtype=np.float64).copy()
    dt = np.float64(np.float32(dt))
    cs, hs = [c.copy()], [h.copy()]
    for a, b, s in np.asarray(cmds, dtype=np.float64):
        g = np.array([b * h[0] - s * h[1], s * h[0] + b * h[1]])
        h = g / np.hypot(g[0], g[1])
        c = c + dt * a * h
        cs.append(c.copy())
        hs.append(h.copy())
    return np.array(cs), np.array(hs)


def one_vehicle_scene(c=(3.0, -2.0), yaw=0.3, vel=(0.0, 0.0), extent=(2.4, 1.0)):
    """A scene dict with no pedestrians and one vehicle, its ring placed as set_dynamic_boxes places it."""
    local = scenarios.ring_local_offsets(*extent)
    c = np.float32(c).astype(np.float64)
    return {"loc": np.zeros((0, 3)), "vel": np.zeros((0, 3)), "dynamic_obstacles": [(c, scenarios.place_ring_f32(c, yaw, local))],
            "dynamic_vel": np.array([vel], dtype=np.float64), "dynamic_yaw": np.array([yaw]), "dynamic_extent": np.array([extent])}


def start_twin(scenes, tracks=None):
    """The twin as the batch is after upload(device_vehicles=True) and set_vehicle_tracks(tracks): the headings are those of the
    boxes (stored BEFORE the tracked vehicles are placed: a keyframe's yaw is not the vehicle's heading), tracked vehicles at tau 0."""
    for k, sc in enumerate(scenes):
        sc["dynamic_heading"] = scenarios.vehicle_headings(sc)
        sc["dynamic_present"] = np.ones(len(sc["dynamic_obstacles"]), bool)
        if tracks is not None:
            scenarios.place_tracked(sc, tracks[k], 0, None)


def drive_twin(scenes, kinds, cmds, dts, tracks, tau):
    """One integrating tick of every scene's twin, arriving at tick ``tau``."""
    for k, sc in enumerate(scenes):
        if len(sc["dynamic_obstacles"]):
            scenarios.drive_vehicles(sc, kinds[k], cmds[k], dts[k], None if tracks is None else tracks[k], tau)
