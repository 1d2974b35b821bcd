"""GPU tests of what a batch and a handle keep between calls: drop a feature and set it again, grow the state, shrink it.

A stale-state check against a fresh object, not a check of values (those are pinned to the oracle elsewhere): an object that has
been through another crowd, with every feature set, dropped and set again, must read back bit for bit what a freshly created one
reads back after the last set of calls alone -- so nothing of the earlier crowd (a buffer, a flag, a capacity, a counter) may
survive a drop or an upload.  The first two tests are the sequence written when a batch ended at steering; the others take every
later feature through three generations of crowds in two profiles (tests/_lifecycle_cases.py), hold the header's drop rules call by
call, make one refused call per feature, and take a handle across the sizes where it changes its kernel path.  Every comparison is
exact.  Run on the MI355X box with  python -m pytest tests -m gpu."""
import re
from functools import lru_cache

import numpy as np
import pytest

import _lifecycle_cases as LC
import test_batch_modes_gpu as M
import test_batch_restart_gpu as R
from carla_social_force_model_amd import replay as _replay
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd._lib import SfmLibraryError, fptr, iptr, u8ptr
from carla_social_force_model_amd.batch import (EP_DONE, EP_REASON, MODE_KEYS, REASON_TIME_LIMIT, SfmBatch, mode_scene_arrays, pack_modes,
                                                pack_route_rows, pack_scenes, pack_tracks)
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


# ---- every batch feature set, dropped, regrown, shrunk (the crowds, call lists and the drop table: tests/_lifecycle_cases.py) ----------
ORDERS = {"A,B,C": (("A", 0), ("B", 0), ("C", 0)),              # grow, then shrink
          "B,A,B'": (("B", 0), ("A", 0), ("B", 1)),             # shrink, then grow into another crowd of B's shape
          "C,C": (("C", 0), ("C", 0))}                          # the same crowd twice: the second upload forgets the first run's counters
VS = LC.VEHICLE_SCENE
SFM_ERR_STATE = -3


def _new_batch():
    """A batch on torch's current stream, so that the views and the downloads are ordered."""
    import torch
    b = SfmBatch(LC.configs(), list(LC.DTS))
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
    except Exception:
        b.close()
        raise
    return b


def _device_mask():
    import torch
    return torch.tensor(np.array([1, 1, 0], np.uint8), dtype=torch.uint8, device="cuda")


def _flat(x):
    """The arrays of a getter's result (tuples, lists and dicts of arrays and numbers), in order."""
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in _flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for e in x for a in _flat(e)]
    return [np.asarray(x)]


def _same_flat(u, v):
    u, v = _flat(u), _flat(v)
    return len(u) == len(v) and all(R._same_array(a, c) for a, c in zip(u, v))


def _assert_all(got, want, what):
    (gs, gw), (ws, ww) = got, want
    assert len(gs) == len(ws), what
    for k in range(len(ws)):
        R._assert_scene(gs[k], ws[k], f"{what}: scene {k}")
    assert gw.keys() == ww.keys(), what
    for name, u in gw.items():
        v = np.asarray(ww[name])
        u = np.asarray(u)
        assert u.shape == v.shape and u.dtype == v.dtype and np.array_equal(u, v, equal_nan=name == "episodes"), f"{what}: {name}"


def _views(b, c, what):
    """Every zero-copy view, fetched now, as a host array -- after it has been held to the download of the same buffer."""
    import torch
    cat = lambda parts, shape: np.concatenate([np.asarray(p) for p in parts]) if len(parts) else np.zeros(shape)
    host = lambda t: t.cpu().numpy()
    out = {}

    def hold(name, tensor, download):
        torch.cuda.synchronize()
        got = host(tensor)
        assert got.shape == download.shape and R._same_array(got, np.asarray(download, got.dtype)), f"{what}: the view {name}"
        out[name] = got

    loc, vel = b.state_arrays()
    hold("state", b.state_tensor(), np.float32(np.stack([loc[:, 0], loc[:, 1], vel[:, 0], vel[:, 1]], axis=1)))
    steer = b.steering()
    hold("command", b.command_tensor(), np.concatenate([cat([s[1] for s in steer], (0, 3)), np.float32(cat([s[0] for s in steer], (0,)))[:, None]], axis=1))
    hold("observation", b.observation_tensor(), cat(b.observations(), (0, 1)))
    hold("scan", b.scan_tensor(), cat(b.scans(), (0, 1)))
    hold("grid", b.grid_tensor(), cat(b.grids(), (0, 1)))
    rec, done = b.episodes()
    hold("episode", b.episode_tensor(), rec)
    hold("done", b.done_tensor(), done.astype(np.uint8))
    hold("reset_count", b.reset_count_tensor(), b.restart_noise()[0].view(np.int32))
    if c["profile"] == "policy":
        drive = b.vehicle_driving()
        hold("vehicle_command", b.vehicle_command_tensor(),
             np.concatenate([cat([d[1] for d in drive], (0, 3)), np.float32(cat([d[0] for d in drive], (0,)))[:, None]], axis=1))
        hold("vehicle_observation", b.vehicle_observation_tensor(), cat(b.vehicle_observations(), (0, 1)))
        hold("vehicle_scan", b.vehicle_scan_tensor(), cat(b.vehicle_scans(), (0, 1)))
        r = c["routes"]
        _, gx, gy = pack_route_rows(r["graph_types"], r["goals"], r["mask"], b.scene_off)
        hold("route_goal", b.route_goal_tensor(), np.stack([gx, gy], axis=1))
        hold("route_status", b.route_status_tensor(), cat([q["status"] for q in b.routes()], (0,)))
    else:
        hold("row_score", b.row_score_tensor(), cat(b.row_scores(), (0, 4)))
        hold("scene_score", b.scene_score_tensor(), b.scene_scores())
    return out


def _something_happened(c, read, restarted):
    """What makes a pass mean something, on the fresh batch of crowd ``c``: ``read`` is its ``read_all``, ``restarted`` per scene the
    positions and steering kinds straight after one more restart of every scene."""
    scenes, whole = read
    dts = np.float32(LC.DTS)
    assert any(not np.array_equal(s["loc"], sc["loc"]) for s, sc in zip(scenes, c["scenes"])), "the ticks moved nobody"
    rec, done = whole["episodes"], whole["done"]
    assert done[1] and rec[1, EP_DONE] == 1.0 and int(rec[1, EP_REASON]) & REASON_TIME_LIMIT, "no episode ended"
    assert whole["resets"][1] >= 1 and whole["resets"][VS] >= 1, whole["resets"]     # ... and was restarted (the vehicle scene by the host)
    # straight after a restart of every scene: a live row that nobody steers is not where the snapshot (the upload) has it
    moved = [(np.float32(loc[:, :2]) != np.float32(sc["loc"][:, :2])).any(axis=1) & (kind == 0) & (np.abs(loc[:, :2]).max(axis=1, initial=0.0) < 1.0e6)
             for (loc, kind), sc in zip(restarted, c["scenes"])]
    assert any(m.any() for m in moved), "the restart noise moved nobody"
    hit = lambda key, width: (any((s[key][:, width:] > 0).any() for s in scenes), any((s[key][:, width:][_scanned(s[key], width)] == 0).any() for s in scenes))
    assert hit("scan", c["scan"]["R"]) == (True, True), "row scans"
    assert any(s["grid"][:, 0].any() for s in scenes) and any(s["grid"][:, 3:].any() for s in scenes), "grids"
    if c["profile"] == "replay":
        assert any((s["row_scores"][c["observed"]["roles"][k] == 2, 0] > 0).any() for k, s in enumerate(scenes)), "no scored row has a sample"
        return
    status = np.concatenate([s["route_status"] for s in scenes])
    length = np.concatenate([s["route_L"] for s in scenes])
    assert ((status == 1) & (length >= 3)).any() and ((status != 1) & (status != 0)).any(), sorted(set(status))
    assert hit("vscan", c["vscan"]["R"]) == (True, True), "vehicle scans"
    ctr0, vel0 = LC.vehicles_of(c)
    v = scenes[VS]
    driven = np.flatnonzero(v["vkind"] != 0)
    assert len(driven)
    for m in driven:                                              # not where it would be after 0 .. 4 ticks of running free
        free = [ctr0[m] + np.float32(t) * dts[VS] * vel0[m] for t in range(5)]
        assert all(np.abs(np.float32(v["ctr"][m]) - f).max() > 1.0e-3 for f in free), f"vehicle {m} is where its free-running copy would be"


def _scanned(rec, R_):
    """The rows of a scan record that were scanned: an unscanned row reads zeros, a scanned one has positive ranges."""
    return (rec[:, :R_] > 0).any(axis=1)


@lru_cache(maxsize=None)
def _fresh(profile, gen, variant):
    """(read_all, views, restarted) of a fresh batch that got ``last_calls`` of one crowd (computed once, shared, never changed);
    ``restarted``: per scene (positions, steering kinds) straight after one more restart of every scene, taken last."""
    c = LC.crowd(profile, gen, variant)
    f = _new_batch()
    try:
        LC.last_calls(f, c, _device_mask())
        read, views = LC.read_all(f, c), _views(f, c, f"fresh {profile} {gen}{variant}")
        f.restart()
        return read, views, [(loc, kind) for (loc, _), (kind, _) in zip(f.state(), f.steering())]
    finally:
        f.close()


def _assert_like_fresh(b, c, variant, what):
    want, want_views, _ = _fresh(c["profile"], c["gen"], variant)
    _assert_all(LC.read_all(b, c), want, what)
    views = _views(b, c, what)
    assert views.keys() == want_views.keys()
    for name, u in views.items():
        assert R._same_array(u, want_views[name]), f"{what}: the view {name}"


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("profile", LC.PROFILES)
def test_reused_batch_equals_a_fresh_one(profile, order):
    """One batch gets ``last_calls`` of every generation in turn, with the drop sequence (rotated per turn and order) in between; a
    fresh batch gets the last generation alone.  Everything read back, and every zero-copy view, is bitwise equal -- and the fresh
    batch's run is not vacuous (``_something_happened``)."""
    gens = ORDERS[order]
    a = _new_batch()
    try:
        mask = _device_mask()
        before = None
        for turn, (gen, variant) in enumerate(gens):
            c = LC.crowd(profile, gen, variant)
            if before is not None:
                for name in LC.drop_sequence(turn + list(ORDERS).index(order)):
                    LC.CALLS[name][1](a, before)
            LC.last_calls(a, c, mask)
            before = c
        gen, variant = gens[-1]
        read, _, restarted = _fresh(profile, gen, variant)
        _something_happened(c, read, restarted)
        _assert_like_fresh(a, c, variant, f"{profile} {order}")
    finally:
        a.close()


def _setup(b, setup):
    """Generation A with everything of the set-up: a profile, or the policy profile with its routes exchanged for a schedule
    ("spawns"; "born": one under which everyone is there from the start)."""
    c = LC.crowd(setup if setup in LC.PROFILES else "policy", "A")
    LC.set_everything(b, c)
    if setup not in LC.PROFILES:
        b.set_routes(None, None, None)
        b.set_spawns(c["scheds"] if setup == "spawns" else [None] * len(LC.DTS))
        b.snapshot()
    return c


def _getter(b, feature):
    return getattr(b, LC.FEATURES[feature][1])


def _assert_gone(b, feature):
    """The feature's getter raises with the feature's own message, and so answers the library itself when asked directly."""
    _, _, message, (symbol, nulls) = LC.FEATURES[feature]
    with pytest.raises(SfmLibraryError, match=re.escape(message)):
        _getter(b, feature)()
    assert getattr(b._lib, symbol)(b._b, *([None] * nulls)) == SFM_ERR_STATE, f"{symbol} does not say that the {feature} are gone"
    assert message in b._lib.sfm_batch_last_error(b._b).decode(), feature


def _delay_probe(b, take):
    """Where the vehicle scene's vehicles are one tick after a restart two ticks behind the snapshot (``take``: taken now), and the
    noise counters."""
    if take:
        b.snapshot()
    _ticks(b, 2)
    b.restart([VS])
    _ticks(b, 1)
    return b.vehicle_tracks(), b.dynamic_obstacles()[VS], b.restart_noise()


def _delay_witness(setup, call, delays, take):
    """A batch set up alike that got the same call and then the noise again, with or without the delays: its probe."""
    w = _new_batch()
    try:
        c = _setup(w, setup)
        LC.CALLS[call][1](w, c)
        w.set_restart_noise(track_delay=c["track_delay"] if delays else None, **c["noise"])
        return _delay_probe(w, take)
    finally:
        w.close()


@pytest.mark.parametrize("call,setup", [(call, setup) for call in LC.CALLS for setup in LC.SETUPS[call]])
def test_drop_table(call, setup):
    """On generation A with everything set: the call, then per feature of its rows in DROPS -- a kept feature's getter returns what it
    returned before (the snapshot: restart goes on working; the delays: a restarted scene's tracked vehicle arrives as late as on a
    batch that was given the delays anew), a dropped feature's getter raises with the feature's own message.  Then ``last_calls`` of
    generation C on this batch equals a fresh batch's: a drop leaves the batch no worse than new."""
    rows = {f: outcome for (name, f), (outcome, _) in LC.DROPS.items() if name == call}
    assert rows
    b = _new_batch()
    try:
        c = _setup(b, setup)
        rows = {f: outcome for f, outcome in rows.items() if f in LC.HOLDS[setup]}     # (the rows this set-up holds: it must answer for each)
        assert rows
        was = {f: _getter(b, f)() for f in rows if LC.FEATURES[f][1] not in (None, "restart")}
        LC.CALLS[call][1](b, c)
        for f, outcome in rows.items():
            if f not in was:
                continue
            if outcome == LC.DROPPED:
                _assert_gone(b, f)
                continue
            now = _getter(b, f)()
            if call in ("set_dynamic_boxes", "set_dynamic_obstacles") and f in ("observations", "scans", "grids"):
                now, old = [x for k, x in enumerate(now) if k != VS], [x for k, x in enumerate(was[f]) if k != VS]     # (the tracked vehicle is back
                assert _same_flat(now, old), f"{call} keeps {f}"                                                       #  where it was uploaded)
            else:
                assert _same_flat(now, was[f]), f"{call} keeps {f}"
        snap = rows.get("snapshot")
        if snap == LC.DROPPED:
            _assert_gone(b, "snapshot")
        tracks_and_noise = True
        try:
            b.vehicle_tracks(), b.restart_noise()
        except SfmLibraryError:
            tracks_and_noise = False
        if "noise delays" in rows and tracks_and_noise:           # (a kept snapshot is the one the probe restarts from)
            kept, take = rows["noise delays"] == LC.KEPT, snap != LC.KEPT
            delayed, on_time = _delay_witness(setup, call, True, take), _delay_witness(setup, call, False, take)
            assert not _same_flat(delayed, on_time)               # (the probe can tell: with the delays the vehicle is elsewhere)
            assert _same_flat(_delay_probe(b, take), delayed if kept else on_time), f"{call}: the delays are {rows['noise delays']}"
        elif snap == LC.KEPT:
            b.restart()
        last = LC.crowd(c["profile"], "C")
        LC.last_calls(b, last, _device_mask())
        _assert_like_fresh(b, last, 0, f"{call} on {setup}, then C")
    finally:
        b.close()


def _refusals(b, c):
    """(what, call): one refused call per feature, each through the library (a raw call returns its code; a method raises, and
    its entry returns 0 if it does not)."""
    L, h = b._lib, b._b
    n, veh = int(b.scene_off[-1]), int(b._dyn[0][-1])
    # (every array has a name: the library is handed addresses, and an array must outlive the call)
    per_scene, one, rows = np.ones(3, np.float32), np.ones(1, np.float32), np.zeros(n, np.float32)
    bad_off = np.ones(4, np.int32)                                 # scene offsets that do not start at 0
    nan = np.full(max(n, veh), np.nan, np.float32)
    no_agent, bad_steps, seeds = np.full(3, -1, np.int32), np.array([0, -1, 0], np.int32), np.zeros(3, np.uint32)
    kind3, driven, unchained, mask2 = np.full(n, 3, np.uint8), np.ones(veh, np.uint8), np.zeros(n, np.uint8), np.array([0, 2, 0], np.uint8)
    out = [
        ("observation k = 0", lambda: L.sfm_batch_set_observation(h, 0, fptr(per_scene), 0)),
        ("vehicle observation k = 0", lambda: L.sfm_batch_set_vehicle_observation(h, 0, fptr(per_scene), 0, None, None, None)),
        ("episodes with a negative max_steps", lambda: L.sfm_batch_set_episodes(h, iptr(no_agent), fptr(per_scene), fptr(per_scene), fptr(per_scene),
                                                                                 iptr(bad_steps))),
        ("scan R = 0", lambda: L.sfm_batch_set_scan(h, 0, fptr(one), fptr(one), fptr(per_scene), fptr(per_scene), fptr(per_scene), None, 0)),
        ("vehicle scan R = 0", lambda: L.sfm_batch_set_vehicle_scan(h, 0, fptr(one), fptr(one), fptr(per_scene), fptr(per_scene), fptr(per_scene),
                                                                    None, 0, 0.0, 0.0)),
        ("grid G = 0", lambda: L.sfm_batch_set_grid(h, 0, fptr(per_scene), None, 0)),
        ("noise tries = 0", lambda: L.sfm_batch_set_restart_noise(h, seeds.ctypes.data, fptr(rows), fptr(rows), None, None, fptr(per_scene),
                                                                  fptr(per_scene), 0, None)),
        ("steering kind 3", lambda: L.sfm_batch_set_steering(h, u8ptr(kind3), fptr(rows), fptr(rows), fptr(rows))),
        ("driving command not finite", lambda: L.sfm_batch_set_vehicle_driving(h, u8ptr(driven), fptr(nan), fptr(nan), fptr(nan))),
        ("spawn time NaN", lambda: L.sfm_batch_set_spawn_schedule(h, fptr(nan), u8ptr(unchained))),
        ("upload with bad scene offsets", lambda: L.sfm_batch_upload_state(h, iptr(bad_off), *([None] * 11))),
        ("boxes with bad scene offsets", lambda: L.sfm_batch_set_dynamic_boxes(h, iptr(bad_off), *([None] * 9))),
        ("rings with bad scene offsets", lambda: L.sfm_batch_set_dynamic_obstacles(h, iptr(bad_off), *([None] * 7))),
        ("params NULL", lambda: L.sfm_batch_set_params(h, None)),
        ("restart mask value 2", lambda: L.sfm_batch_restart(h, u8ptr(mask2))),
        ("end_step flag 2", lambda: L.sfm_batch_end_step(h, 2)),
    ]
    track = pack_tracks(c["tracks"], b._dyn[0])
    track["kx"] = track["kx"].copy()
    track["kx"][0] = np.inf
    out.append(("track keyframe not finite", lambda: (b.set_vehicle_tracks(track), 0)[1]))      # (a method that does not raise: 0, not refused)
    # a role of 3 (a 3-D batch and one with modes refuse observed tracks before they look at the roles: still a refusal)
    if c["profile"] == "replay":
        ob = c["observed"]
        off, frames, obs, role, v0 = _replay.pack_observed(ob["tracks"], ob["roles"], b.scene_off, ob["v0"])
        role = role.copy()
        role[0] = 3
        out.append(("role 3", lambda: L.sfm_batch_set_observed(h, off.ctypes.data, iptr(frames), fptr(obs), u8ptr(role), fptr(v0), 1)))
    else:
        out.append(("route capacity 65", lambda: (b.set_routes(**dict(c["routes"], capacity=65)), 0)[1]))
        pm = pack_modes(c["plans"], b.scene_off, c["scenes"])
        mode = pm["mode"].copy()
        mode[0] = 5
        despawn, t0, thr = mode_scene_arrays(3, True, list(LC.T0), 2.0)
        out.append(("mode 5", lambda: L.sfm_batch_set_mode_fsm(h, u8ptr(mode), *(fptr(pm[k]) for k in MODE_KEYS[1:]), iptr(pm["wp_offsets"]),
                                                               fptr(pm["wp_x"]), fptr(pm["wp_y"]), u8ptr(pm["wp_crossing"]), iptr(despawn),
                                                               fptr(t0), fptr(thr), fptr(pm["first_vehicle_extent"]))))
    return out


FLAGS = ("has_snapshot", "obs_k", "has_episodes", "scan_rays", "grid_cells", "has_restart_noise", "observed_every", "driving", "vobs_k",
         "vscan_rays", "route_capacity", "planar")           # what the Python object itself remembers of the features


@pytest.mark.parametrize("profile", LC.PROFILES)
def test_a_refused_call_drops_nothing(profile):
    """Generation B with everything set, two ticks; then one refused call per feature.  Everything read back is what it was, bit for
    bit, and one more tick gives what it gives on a batch that was never refused anything."""
    c = LC.crowd(profile, "B")
    b, f = _new_batch(), _new_batch()
    try:
        for x in (b, f):
            LC.set_everything(x, c)
            LC.run(x, c, 0, 2)
        was = LC.read_all(b, c)
        flags = [getattr(b, name) for name in FLAGS]
        for what, call in _refusals(b, c):
            try:
                rc = call()
            except SfmLibraryError:
                rc = -1
            assert rc != 0, f"{what} was not refused"
        assert [getattr(b, name) for name in FLAGS] == flags
        _assert_all(LC.read_all(b, c), was, f"{profile}: after the refusals")
        for x in (b, f):
            LC.run(x, c, 2, 1)
            LC.sense(x, c)
        _assert_all(LC.read_all(b, c), LC.read_all(f, c), f"{profile}: a tick after the refusals")
    finally:
        b.close()
        f.close()


# ---- one handle across the sizes where it changes its kernel path -----------------------------------------------------------------
PATHS = ("listed", "packed", "general", "lean", "small")


@lru_cache(maxsize=None)
def _path_crowd(name):
    """(crowd, config, mode plan or None) per kernel path: N = 4160 planar with all forces (rows packed, the tile-pair list on above
    4096); N = 2112 in 3-D with radii, two device-side vehicles and modes (rows packed; the modes keep a handle off the fused tick, so
    this is the pair kernel and its epilogue); the same shape without modes (the fused general form, rows packed); N = 1024 planar with
    the acceleration and the pedestrian force only (the lean fused form); N = 300 with all forces (no packing)."""
    geo = dict(n_borders=6, n_static=2, n_dynamic=2, border_len=(5.0, 20.0))
    cfg = default_sfm_config()
    modes = None
    if name == "listed":
        sc = scenarios.make_scenario(4160, 41, **geo)
    elif name == "packed":
        sc = scenarios.make_scenario(2112, 42, z_spread=1.5, **geo)
        cfg["use_ped_radius"] = True
        modes = scenarios.make_mode_plan(sc, 47)                  # (moves the first waypoints: once, here)
    elif name == "general":
        sc = scenarios.make_scenario(2112, 45, z_spread=1.5, **geo)
        cfg["use_ped_radius"] = True
    elif name == "lean":
        sc = scenarios.make_scenario(1024, 43)
        cfg = default_sfm_config(("acceleration_force", "pedestrian_force"))
    else:
        sc = scenarios.make_scenario(300, 44, **geo)
    return sc, cfg, modes


def _path_run(eng, name):
    sc, cfg, modes = _path_crowd(name)
    eng.set_params(cfg, 0.05)
    eng.set_borders(sc.borders, sc.border_centers, sc.border_lengths)
    eng.set_static_obstacles(sc.static_obstacles)
    if sc.dynamic_obstacles:
        eng.set_dynamic_boxes([c for c, _ in sc.dynamic_obstacles], sc.dynamic_yaw, sc.dynamic_extent, sc.dynamic_vel)
    else:
        eng.set_dynamic_boxes([], [], [], [])
    eng.upload_state(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, None)
    eng.set_waypoint_stream(sc.seed, 0.3 * sc.world_side, 2.0)
    if modes is not None:
        plan, managers = modes
        eng.set_mode_fsm(managers, plan["queues"], despawn_on_arrival=True, sim_time0=0.0, first_vehicle_extent=sc.dynamic_extent[0])
    eng.run(8, redraw=modes is None)


def _path_read(eng, name):
    loc, vel, wp = eng.state()
    out = {"loc": loc, "vel": vel, "wp": wp, "v": eng.velocities(), "draws": eng.draw_counts()}
    if _path_crowd(name)[2] is not None:
        out.update(zip(("mode", "target", "cursor"), eng.modes()))
    return out, (eng.kernel_variant(), eng.fused_form(), eng.timing()[2], eng.pair_work()[0])


@pytest.mark.parametrize("last", PATHS)
def test_handle_across_its_kernel_paths(last, monkeypatch):
    """One handle runs the five crowds, ``last`` last and the other four before it in their order; a fresh handle runs ``last``
    alone.  State, velocities, waypoints, draw counters and modes are bitwise equal, and so are the kernel the last run launched, its
    fused form, its number of launches and the pair kernel's work items (the tile-pair list): a path chosen for an earlier crowd
    shows even where the numbers agree."""
    monkeypatch.setenv("SFM_RESORT_EVERY", "3")                   # (read when a handle is created)
    a, f = SfmEngine(default_sfm_config(), 0.05, device=0), SfmEngine(default_sfm_config(), 0.05, device=0)
    try:
        a.set_timing(True)
        f.set_timing(True)
        for name in [p for p in PATHS if p != last] + [last]:
            _path_run(a, name)
        _path_run(f, last)
        (got, got_path), (want, want_path) = _path_read(a, last), _path_read(f, last)
        assert got_path == want_path, (got_path, want_path)
        assert got.keys() == want.keys()
        for name, u in got.items():
            assert R._same_array(u, want[name]), f"{last}: {name}"
        assert not np.array_equal(want["loc"], _path_crowd(last)[0].loc)                   # (the run moved the crowd)
        # ... and the fresh handle took the path the crowd was made for: the tile-pair list above 4096 rows only (fewer work items than
        # the triangle of 64-row tiles), the pair kernel under modes and above 4096, the fused tick's two forms elsewhere
        tiles = (_path_crowd(last)[0].n + 63) // 64
        whole = tiles * (tiles - 1) // 2 + (tiles + 1) // 2
        assert (want_path[3] < whole) == (last == "listed") and want_path[3] <= whole, (want_path, whole)
        form = {"listed": "none", "packed": "none", "general": "sfm_fused_tick_kernel<general>", "lean": "sfm_fused_tick_kernel<lean>",
                "small": "sfm_fused_tick_kernel<general>"}[last]
        assert want_path[1] == form and ("sfm_pair_sym_kernel" in want_path[0]) == (form == "none"), want_path
    finally:
        a.close()
        f.close()
