"""GPU tests of what a batch and a handle keep between calls: drop a feature and set it again, grow the state.

A stale-state check against a fresh object, not a check of values (those are pinned to the oracle elsewhere): an object that has
been through another crowd, with every feature set, dropped and set again, must read back bit for bit what a freshly created one
reads back after the last set of calls alone -- so nothing of the earlier crowd (a buffer, a flag, a capacity, a counter) may
survive a drop or an upload.  Run on the MI355X box with  python -m pytest tests -m gpu."""
import numpy as np
import pytest

import test_batch_modes_gpu as M
import test_batch_restart_gpu as R
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd._lib import SfmLibraryError, fptr, iptr
from carla_social_force_model_amd.batch import SfmBatch, pack_scenes
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.engine import SfmEngine

pytestmark = pytest.mark.gpu

DTS = (0.05, 0.04, 0.05)
T0 = (4.5, 4.5, 4.7)
SMALL = (0, 5, 70)                   # an empty scene, one below a wave, one across a wave boundary
LARGE = (3, 70, 130)                 # every scene grows; the state arrays are allocated again
VEHICLE_SCENE = 2                    # the scene with the two vehicles, the first of them on a track
TICKS = 8                            # what the track plans cover


def _crowd(sizes, seed):
    """Scenes, mode plans, spawn schedules, tracks, steering kinds and commands of one 3-D crowd."""
    made = [M._scene(n, seed + k, 2 if k == VEHICLE_SCENE else 0, z_spread=1.5, borders=2) for k, n in enumerate(sizes)]
    scenes = [m[0] for m in made]
    plans = [scenarios.make_mode_plan(sc, seed + 50 + k, queue_len=1)[0] for k, sc in enumerate(scenes)]
    scheds = [scenarios.make_spawn_plan(sc, seed + 70 + k, dt=DTS[k], t0=T0[k], present=0.35, horizon=1.5) for k, sc in enumerate(scenes)]
    tracked = scenarios.make_track_plan(scenes[VEHICLE_SCENE], seed + 90, TICKS, dt=DTS[VEHICLE_SCENE])
    tracks = [[tracked[0], None] if k == VEHICLE_SCENE else None for k in range(len(sizes))]
    rng = np.random.default_rng(seed + 99)
    kinds = [rng.integers(0, 3, n) for n in sizes]
    cmds = [np.float32(rng.uniform(-1.5, 1.5, (n, 3))) for n in sizes]
    return scenes, plans, scheds, tracks, kinds, cmds


def _set_everything(b, crowd):
    scenes, plans, scheds, tracks, kinds, cmds = crowd
    b.upload(scenes, device_vehicles=True)
    assert not b.planar
    b.set_vehicle_tracks(tracks)
    b.set_modes(plans, despawn_on_arrival=True, sim_time0=list(T0), arrive_thresholds=2.0, scenes=scenes)
    b.set_spawns(scheds)
    b.set_steering(kinds, cmds)
    b.snapshot()


def _ticks(b, n):
    for _ in range(n):
        b.tick(integrate=True)


def _last_calls(b, crowd):
    """Step 3: the larger crowd with every feature, three ticks, scene 1 back to the snapshot, one more tick."""
    _set_everything(b, crowd)
    _ticks(b, 3)
    b.restart([1])
    _ticks(b, 1)


def _read(b):
    """Everything a batch hands back, per scene: state, waypoints and draw counters, vehicles, modes and clocks, births, track
    presence, steering; and the tracks' tick counter."""
    out = [{"loc": loc, "vel": vel, "wp": wp, "draws": d, "ctr": [c for c, _ in veh], "ring": [r for _, r in veh]}
           for (loc, vel), (wp, d), veh in zip(b.state(), b.waypoints(), b.dynamic_obstacles())]
    clocks = b.clocks()
    tick, present = b.vehicle_tracks()
    for k, ((m, t, c), (born, when), p, (kd, cmd)) in enumerate(zip(b.modes(), b.spawns(), present, b.steering())):
        out[k].update(mode=m, target=t, cursor=c, clock=clocks[k:k + 1], born=born, birth=when, present=p, kind=kd, cmd=cmd)
    return out, tick


def test_batch_after_drops_and_growth_equals_a_fresh_one():
    """B = 3, 3-D, two device-side vehicles in one scene, one of them tracked.  (1) scenes of 0, 5 and 70 rows with modes, a spawn
    schedule, steering and a snapshot, three ticks; (2) steering dropped, then the modes (which takes the schedule along), then
    the boxes (which takes the tracks along), one tick; (3) scenes of 3, 70 and 130 rows, every feature again, three ticks, scene 1
    restarted from the new snapshot, one tick.  A fresh batch gets (3) alone; everything read back is bitwise equal."""
    small, large = _crowd(SMALL, 5100), _crowd(LARGE, 5200)
    cfgs = [M._config(k) for k in range(len(DTS))]
    a, f = SfmBatch(cfgs, list(DTS)), SfmBatch(cfgs, list(DTS))
    try:
        _set_everything(a, small)
        _ticks(a, 3)
        a.set_steering(None)
        with pytest.raises(SfmLibraryError):
            a.steering()
        a.set_modes(None)
        for gone in (a.modes, a.spawns):                         # the schedule went with the modes
            with pytest.raises(SfmLibraryError):
                gone()
        dy = pack_scenes(small[0])["dynamic"]                    # the vehicles as rings that stay where they are: no boxes
        a._check_drops(a._lib.sfm_batch_set_dynamic_obstacles(a._b, *(iptr(x) for x in dy[:2]), *(fptr(x) for x in dy[2:])),
                       "sfm_batch_set_dynamic_obstacles")
        for gone in (a.vehicle_tracks, a.restart):               # the tracks went with the boxes, and the snapshot with both
            with pytest.raises(SfmLibraryError):
                gone()
        _ticks(a, 1)
        _last_calls(a, large)
        _last_calls(f, large)
        (got, got_tick), (want, want_tick) = _read(a), _read(f)
        assert got_tick == want_tick == 4
        for k in range(len(LARGE)):
            R._assert_scene(got[k], want[k], f"scene {k}")
        assert not np.array_equal(want[VEHICLE_SCENE]["loc"], large[0][VEHICLE_SCENE]["loc"])      # (the ticks moved the rows)
    finally:
        a.close()
        f.close()


def _handle_crowd(n, seed, geometry):
    return scenarios.make_scenario(n, seed, n_borders=6 if geometry else 0, n_dynamic=2 if geometry else 0, border_len=(5.0, 20.0))


def _handle_run(eng, sc):
    eng.set_borders(sc.borders, sc.border_centers, sc.border_lengths)
    if sc.dynamic_obstacles:
        eng.set_dynamic_boxes([c for c, _ in sc.dynamic_obstacles], sc.dynamic_yaw, sc.dynamic_extent, sc.dynamic_vel)
    else:
        eng.set_dynamic_boxes([], [], [], [])
    eng.upload_state(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, None)
    eng.run(2)


def test_handle_after_growth_equals_a_fresh_one():
    """N = 64, run(2); N = 200 with borders and two device-side vehicles, run(2); N = 64 without them again, run(2): state and
    velocities bitwise equal to a fresh handle's that was given the last crowd only."""
    first, big, last = _handle_crowd(64, 31, False), _handle_crowd(200, 32, True), _handle_crowd(64, 33, False)
    cfg = default_sfm_config()
    a, f = SfmEngine(cfg, 0.05, device=0), SfmEngine(cfg, 0.05, device=0)
    try:
        for sc in (first, big, last):
            _handle_run(a, sc)
        _handle_run(f, last)
        (loc_a, vel_a), (loc_f, vel_f) = a.state()[:2], f.state()[:2]
        assert np.array_equal(loc_a, loc_f) and np.array_equal(vel_a, vel_f)
        assert np.array_equal(a.velocities(), f.velocities())
        assert not np.array_equal(loc_f, last.loc)               # (the run moved the crowd)
    finally:
        a.close()
        f.close()
