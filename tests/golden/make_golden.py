#!/usr/bin/env python3
"""Generate the golden vectors in tests/golden/*.npz by running the REFERENCE's own NumPy modules.

The reference's outputs need the upstream checkout (UPSTREAM_REFERENCE); --inputs-only does not.
It imports the reference modules that import cleanly here -- stateutils, ped_mode_manager,
pedestrian_state, forces -- and executes *their* code on seeded inputs:

  per-force outputs      forces.{Acceleration,Pedestrian,Border,Obstacle}Force.get_force(PedState)
  summed force           in the dict order of PedestrianSimulation.init_forces (pedestrian_simulation.py:37-48)
  new velocities         stateutils.cap_velocity(vel + dt*F, PedState.max_speed())  (pedestrian_simulation.py:120-121)
  trajectories           20 CARLA-free ticks: forces -> v' -> arrival test (pedestrian_simulation.py:92-95)
                         -> waypoint swap from a pre-drawn queue -> loc += v'*dt

pedestrian_simulation.py itself is not imported (it pulls check_traffic -> shapely, absent in this image);
the three glue lines above call the reference functions it calls, in its order.

Usage:  python tests/golden/make_golden.py                      (rewrites every fixture)
        python tests/golden/make_golden.py --out DIR NAME ...   (only the named cases, into DIR)
        python tests/golden/make_golden.py --inputs-only --out DIR NAME ...
                                        (the inputs of the named cases alone -- scenarios, config, waypoint queues -- built
                                         by this project's code without the upstream checkout: what tests/test_golden_regen.py
                                         compares with the committed fixtures to catch generator drift)
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("UPSTREAM_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from carla_social_force_model_amd import scenarios          # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402
import _golden_io as gio                         # noqa: E402
import _param_sets as psets                      # noqa: E402

DT = 0.05
ARRIVE_THR = 2.0       # run_simulation.py:39 default waypoint_threshold
TRAJ_TICKS = 20
QUEUE = 3


def build_ref_state(sc, cfg):
    peds = PedState(cfg)
    for i in range(sc.n):
        name = f"ped_{i}"
        mm = PedModeManager(name, float(sc.target_speed[i]), PedMode.WALKING_SIDEWALK, 1.5, 1.5)
        m = int(sc.mode[i])
        if m == PedMode.IDLE:
            mm.set_mode(PedMode.IDLE)
        elif m == PedMode.CROSSING_ROAD:
            mm.set_mode(PedMode.CROSSING_ROAD)       # -> CHECKING_TRAFFIC
            mm.set_mode(PedMode.CROSSING_ROAD)       # -> CROSSING_ROAD
        elif m == PedMode.ROAD_TO_SIDEWALK:
            mm.set_mode(PedMode.CROSSING_ROAD)
            mm.set_mode(PedMode.CROSSING_ROAD)
            mm.set_mode(PedMode.WALKING_SIDEWALK)    # -> ROAD_TO_SIDEWALK
        elif m == PedMode.CHECKING_TRAFFIC:
            mm.set_mode(PedMode.CROSSING_ROAD)
        assert int(mm.current_mode) == m
        peds.add_pedestrian((name, 100 + i, sc.loc[i], sc.vel[i], sc.waypoint[i], mm,
                             float(sc.radius[i]), float(sc.target_speed[i])))
    return peds


def build_ref_forces(sc, cfg):
    act = cfg["forces"]
    fd = {}
    if act.get("acceleration_force"):
        fd["acceleration_force"] = ref_forces.AccelerationForce(DT, cfg)
    if act.get("pedestrian_force"):
        fd["pedestrian_force"] = ref_forces.PedestrianForce(DT, cfg)
    if act.get("border_force"):
        fd["border_force"] = ref_forces.BorderForce(DT, cfg, sc.borders,
                                                    sc.section_info() if sc.borders else np.empty((0, 2), object))
    if act.get("static_obstacle_force"):
        f = ref_forces.ObstacleForce(DT, cfg)
        if sc.static_obstacles:
            f.update_obstacles(sc.static_obstacles)
        fd["static_obstacle_force"] = f
    if act.get("dynamic_obstacle_force"):
        f = ref_forces.ObstacleForce(DT, cfg, True)
        if sc.dynamic_obstacles:
            f.update_obstacles(sc.dynamic_obstacles)
            f.update_obstacle_velocities(sc.dynamic_vel)
        fd["dynamic_obstacle_force"] = f
    return fd


def ref_tick(peds, fd):
    """Numeric part of PedestrianSimulation.tick: apply modes, sum forces, cap."""
    peds.apply_current_mode()
    per = {k: f.get_force(peds) for k, f in fd.items()}
    total = sum(per.values()) if per else np.zeros((peds.size(), 3))
    desired = peds.vel() + DT * total
    v_new = ref_stateutils.cap_velocity(desired, peds.max_speed())
    return per, total, v_new


OUT_DIR = HERE
ONLY = None            # None = every case; otherwise the set of case names to (re)generate
INPUTS_ONLY = False    # True: write the inputs alone (no reference code runs)


def import_reference():
    """The reference modules, imported from the upstream checkout; False when it is not present."""
    global ref_forces, ref_stateutils, PedMode, PedModeManager, PedState
    if not os.path.isdir(REF):
        return False
    sys.path.insert(0, REF)
    import forces as ref_forces                      # noqa: E402  (reference)
    import stateutils as ref_stateutils              # noqa: E402  (reference)
    from ped_mode_manager import PedMode, PedModeManager   # noqa: E402  (reference)
    from pedestrian_state import PedState            # noqa: E402  (reference)
    return True


def waypoint_queue(sc):
    rng = np.random.default_rng(sc.seed + 31337)
    return scenarios._f32(rng.uniform(0.0, max(sc.world_side, 1.0), (sc.n, QUEUE, 2)))


def make_case(name, sc, cfg, trajectory=True, dt=None):
    """``dt``: this case's step length (the reference's forces and its velocity update receive it); None = the generator's DT."""
    global DT
    if ONLY is not None and name not in ONLY:
        return
    if dt is not None:
        keep, DT = DT, dt
        try:
            return make_case(name, sc, cfg, trajectory)
        finally:
            DT = keep
    out = gio.encode_inputs(sc, cfg, DT)
    if INPUTS_ONLY:
        # (a full run writes the queue only when the reference's v' is finite: trajectory cases whose v' is not get none)
        if trajectory:
            out["wp_queue"] = waypoint_queue(sc)
        np.savez_compressed(os.path.join(OUT_DIR, name + ".npz"), **out)
        return
    with np.errstate(all="ignore"):
        peds = build_ref_state(sc, cfg)
        fd = build_ref_forces(sc, cfg)
        per, total, v_new = ref_tick(peds, fd)
    out["mode_target_speed"] = peds.target_speed().astype(np.float64)
    for k, v in per.items():
        out["ref_" + k] = np.asarray(v, dtype=np.float64)
    out["ref_total"] = np.asarray(total, dtype=np.float64)
    out["ref_new_vel"] = np.asarray(v_new, dtype=np.float64)
    d = peds.next_waypoint()[:, :2] - peds.loc()[:, :2]
    out["ref_arrived"] = (np.linalg.norm(d, axis=-1) < ARRIVE_THR)

    if trajectory and np.all(np.isfinite(v_new)):
        queue = waypoint_queue(sc)
        out["wp_queue"] = queue
        used = np.zeros(sc.n, dtype=np.int64)
        locs, vels, wps = [], [], []
        with np.errstate(all="ignore"):
            for _ in range(TRAJ_TICKS):
                _, _, v_new = ref_tick(peds, fd)
                peds.state["vel"] = v_new                      # what the ['id','vel'] view write does (:123-124)
                d = peds.next_waypoint()[:, :2] - peds.loc()[:, :2]
                hit = np.linalg.norm(d, axis=-1) < ARRIVE_THR
                for i in np.nonzero(hit)[0]:
                    used[i] += 1
                    peds.state["next_waypoint"][i, :2] = queue[i, (used[i] - 1) % QUEUE]
                peds.state["loc"] = peds.state["loc"] + DT * peds.state["vel"]
                locs.append(peds.loc().copy())
                vels.append(peds.vel().copy())
                wps.append(peds.next_waypoint().copy())
        out["ref_traj_loc"] = np.array(locs)
        out["ref_traj_vel"] = np.array(vels)
        out["ref_traj_wp"] = np.array(wps)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"  {name}: N={sc.n} forces={list(per)} -> {os.path.getsize(path)//1024} KiB")


def main():
    if INPUTS_ONLY:
        print(f"inputs only, numpy {np.__version__}")
    elif not import_reference():
        print(f"make_golden: reference checkout {REF} not present -- nothing to do")
        return
    else:
        print(f"reference at {REF}, numpy {np.__version__}")
    full = default_sfm_config()
    # seeds x sizes, all five forces, stock parameters
    for seed in (0, 1, 2):
        for n in (2, 3, 16, 64, 256):
            sc = scenarios.make_scenario(n, seed * 100 + n, n_borders=max(2, n // 8), n_static=max(1, n // 16),
                                         n_dynamic=max(1, n // 32), border_len=(3.0, 15.0))
            make_case(f"all_s{seed}_n{n}", sc, full, trajectory=(n <= 64))

    # N = 1: zero pedestrian force, everything else still acts
    make_case("single_ped", scenarios.make_scenario(1, 11, 2, 1, 1, border_len=(3.0, 8.0)), full)

    # use_ped_radius = true
    cfg = copy.deepcopy(full)
    cfg["use_ped_radius"] = True
    make_case("radius_n64", scenarios.make_scenario(64, 21, 8, 4, 2, border_len=(3.0, 15.0)), cfg)

    # non-zero z and v_z (3-component ped geometry)
    make_case("zspread_n64", scenarios.make_scenario(64, 31, 8, 4, 2, z_spread=1.5, border_len=(3.0, 15.0)), full)

    # modes: crossing road / road->sidewalk mask the border force; idle / checking-traffic have target 0
    n = 32
    modes = np.ones(n, dtype=np.int64)
    modes[3], modes[7], modes[11], modes[19] = 2, 3, 0, 4
    make_case("modes_n32", scenarios.make_scenario(n, 41, 6, 3, 1, border_len=(3.0, 12.0), modes=modes), full)

    # tight perception thresholds so the obstacle cull actually culls in a small world
    cfg = copy.deepcopy(full)
    cfg["static_obstacle_force"]["perception_threshold"] = 4.0
    cfg["dynamic_obstacle_force"]["perception_threshold"] = 6.0
    make_case("tightcull_n64", scenarios.make_scenario(64, 51, 8, 8, 4, border_len=(2.0, 6.0)), cfg)

    # no geometry at all: obstacle forces that never received obstacles return zeros (forces.py:209-210).
    # (BorderForce cannot even be constructed with an empty border list -- np.vstack([]) at forces.py:131 --
    # so the border force is switched off here; the facade returns zeros in that case.)
    cfg = copy.deepcopy(full)
    cfg["forces"]["border_force"] = False
    make_case("nogeom_n16", scenarios.make_scenario(16, 61), cfg)

    # pedestrian + acceleration force only (BASELINE config 2 at a size the reference can run)
    cfg = default_sfm_config(("acceleration_force", "pedestrian_force"))
    make_case("c2_small_n256", scenarios.make_scenario(256, 1002), cfg, trajectory=False)

    # pedestrian force only (BASELINE config 4 shape)
    cfg = default_sfm_config(("pedestrian_force",))
    make_case("c4_small_n128", scenarios.make_scenario(128, 1004), cfg, trajectory=False)

    # BASELINE config 1 itself: N=64, 40 borders, 16 static, 4 dynamic, all forces
    sc, _ = scenarios.baseline_scenario("c1")
    make_case("c1_n64", sc, full)

    # degenerate: a coincident pair with equal velocities (NaN for both, forces.py:97,105) and a
    # coincident pair with different velocities (finite, theta = -angle(t))
    sc = scenarios.make_scenario(8, 71)
    sc.loc[1] = sc.loc[0]
    sc.vel[1] = sc.vel[0]
    sc.loc[5] = sc.loc[4]
    cfg = default_sfm_config(("acceleration_force", "pedestrian_force"))
    make_case("coincident_n8", sc, cfg, trajectory=False)

    # code-side defaults: tables present but empty (forces.py getters fall back to 3.0/0.1 etc.)
    cfg = default_sfm_config()
    for k in ("pedestrian_force", "border_force", "static_obstacle_force", "dynamic_obstacle_force"):
        cfg[k] = {}
    make_case("defaults_n16", scenarios.make_scenario(16, 81, 3, 2, 1, border_len=(3.0, 8.0)), cfg, trajectory=False)

    # parameter sets away from the stock file (tests/_param_sets.py): every set with use_ped_radius off and on, all five forces,
    # generic velocities; one set in 3-D; the integration set at a second, finer step length
    for k, name in enumerate(psets.NAMES):
        for rad in (False, True):
            n = 48 if rad else 32
            sc = scenarios.make_scenario(n, 9100 + 10 * k + rad, n_borders=6, n_static=3, n_dynamic=2, border_len=(3.0, 12.0))
            make_case(f"ps_{name}{'_rad' if rad else ''}_n{n}", sc, psets.config(name, use_ped_radius=rad), dt=psets.step_of(name))
    sc = scenarios.make_scenario(64, 9171, n_borders=8, n_static=4, n_dynamic=2, z_spread=1.5, border_len=(3.0, 15.0))
    make_case("ps_longrange_z_n64", sc, psets.config("longrange"))
    sc = scenarios.make_scenario(48, 9172, n_borders=6, n_static=3, n_dynamic=2, z_spread=1.5, border_len=(3.0, 12.0))
    make_case("ps_shortrange_z_rad_n48", sc, psets.config("shortrange", use_ped_radius=True))
    sc = scenarios.make_scenario(32, 9173, n_borders=6, n_static=3, n_dynamic=2, border_len=(3.0, 12.0))
    make_case("ps_integrate_fine_n32", sc, psets.config("integrate_fine"), dt=psets.step_of("integrate_fine"))


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv and argv[0] == "--inputs-only":
        INPUTS_ONLY = True
        argv = argv[1:]
    if argv and argv[0] == "--out":
        OUT_DIR = argv[1]
        ONLY = set(argv[2:]) or None
    main()
