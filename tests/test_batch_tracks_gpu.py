"""GPU tests of the batch's vehicle tracks (sfm_batch_set_vehicle_tracks, sfm_batch_download_vehicle_tracks; SfmBatch.
set_vehicle_tracks / vehicle_tracks): the vehicles against the host twin scenarios.place_tracked bit for bit, the tick against the
oracle with the twin's geometry (absent vehicles left out), tracks that restate free running, the mode machine seeing the traffic
come and go, the run forms against each other, batch invariance, switching and refused input.  Built on the recipes of
test_batch_vehicles_gpu.py and test_batch_modes_gpu.py.  Run on the MI355X box with  python -m pytest tests -m gpu."""
import numpy as np
import pytest

import _param_sets
import _parity as P
import test_batch_modes_gpu as M
import test_batch_spawns_gpu as S
import test_batch_vehicles_gpu as V
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import SfmBatch, pack_boxes, pack_scenes, pack_tracks
from carla_social_force_model_amd.spawner import MODE_UNBORN
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

ALL, NO_DYN = V.ALL, V.NO_DYN


def _track(rng, L, first, around, yaw=None):
    """A slow drive (speeds <= 1.4) of L keyframes that starts near ``around``."""
    yaw = rng.uniform(-np.pi, np.pi) + np.cumsum(rng.uniform(-0.05, 0.05, L)) if yaw is None else np.asarray(yaw, dtype=np.float64)
    speed = rng.uniform(0.2, 1.4, L)
    step = 0.05 * speed[:, None] * np.column_stack((np.cos(yaw), np.sin(yaw)))
    xy = np.asarray(around, dtype=np.float64) + rng.uniform(-1.0, 1.0, 2) + np.cumsum(step, axis=0)
    return {"xy": xy, "yaw": yaw, "speed": speed, "first_tick": int(first)}


def _mid(sc):
    return sc["loc"][:, :2].mean(axis=0) if len(sc["loc"]) else np.array([5.0, 5.0])


def _tracked(scenes, cfgs, dts, tracks, planar=None):
    b = V._batch(scenes, cfgs, dts, planar)
    b.set_vehicle_tracks(tracks)
    return b


def _twin(scenes, tracks, tau, dts=None):
    for k, sc in enumerate(scenes):
        scenarios.place_tracked(sc, tracks[k], tau, None if dts is None else dts[k])


def _check_twin(b, scenes, tau, what):
    tick, present = b.vehicle_tracks()
    assert tick == tau, what
    for k, (sc, dev) in enumerate(zip(scenes, b.dynamic_obstacles())):
        V._same_vehicles(dev, sc, f"{what}: scene {k}")
        assert np.array_equal(present[k], sc["dynamic_present"]), f"{what}: scene {k} presence"


def _twin_case():
    counts, sizes = (0, 1, 4, 6, 4, 1), (30, 20, 64, 100, 0, 40)
    scenes = [V._scene(n, 1300 + k, m, slow=False) for k, (n, m) in enumerate(zip(sizes, counts))]
    scenes[1]["dynamic_extent"] = np.array([[0.1, 0.1]])                 # a 6-point ring (the others: 68 points, two lane passes)
    V._restart_twin(scenes[1])
    assert len(scenes[1]["dynamic_obstacles"][0][1]) == 6 and len(scenes[2]["dynamic_obstacles"][0][1]) == 68
    cfgs = [V._config(k, NO_DYN if k == 2 else ALL) for k in range(6)]
    dts = [0.05, 0.04, 0.02, 0.05, 0.03, 0.05]
    rng = np.random.default_rng(77)
    m = [_mid(sc) for sc in scenes]
    sweep = np.linspace(2.9, 3.5, 15)
    sweep = np.where(sweep > np.pi, sweep - 2.0 * np.pi, sweep)              # through +-pi
    tracks = [None,
              [_track(rng, 1, 0, m[1])],                                     # L = 1
              [_track(rng, 20, -3, m[2]), _track(rng, 12, 0, m[2]),          # under way; ends at the last tick of the run
               _track(rng, 4, 5, m[2]), None],                              # enters late and ends inside it; untracked
              [_track(rng, 15, 0, m[3], yaw=sweep), _track(rng, 9, -3, m[3]), _track(rng, 30, 5, m[3]), None,
               _track(rng, 3, 2, m[3]), _track(rng, 1, 11, m[3])],           # six vehicles: the wave stride of 4
              [_track(rng, 6, 0, m[4]), None, _track(rng, 10, 5, m[4]), _track(rng, 8, -3, m[4])],    # no pedestrians
              None]
    return scenes, cfgs, dts, tracks


def test_vehicles_follow_the_twin():
    """Before each of 12 run(1) and after the last, every scene's vehicles (centres, rings) and presence equal place_tracked at
    that tau bit for bit; untracked vehicles move by their scene's dt as ever."""
    scenes, cfgs, dts, tracks = _twin_case()
    b = _tracked(scenes, cfgs, dts, tracks)
    try:
        seen = set()
        for t in range(13):
            _twin(scenes, tracks, t, dts if t else None)
            _check_twin(b, scenes, t, f"tick {t}")
            seen |= {(k, j, bool(p)) for k, sc in enumerate(scenes) for j, p in enumerate(sc["dynamic_present"])}
            if t < 12:
                b.run(1)
        for k, j in ((2, 2), (3, 4), (3, 5), (4, 2)):                         # came or went inside the run
            assert (k, j, True) in seen and (k, j, False) in seen
    finally:
        b.close()


def _oracle_case(z_spread):
    sizes, counts = (64, 30, 1, 0, 200), (4, 2, 1, 3, 2)
    scenes = [V._scene(n, 1700 + k, m, z_spread) for k, (n, m) in enumerate(zip(sizes, counts))]
    cfgs = [V._config(k, ALL) for k in range(5)]
    cfgs[1] = _param_sets.config("longrange", ALL, use_ped_radius=True)
    dts = [0.05, 0.04, 0.05, 0.02, 0.03]
    rng = np.random.default_rng(78)
    m = [_mid(sc) for sc in scenes]
    tracks = [[_track(rng, 4, 3, m[0]), _track(rng, 10, 4, m[0]), _track(rng, 2, 3, m[0]), _track(rng, 3, 5, m[0])],   # ticks 0-2: nobody
              [_track(rng, 8, -3, m[1]), _track(rng, 2, 6, m[1])],           # long-range set; tick 5: nobody
              None,                                                          # untracked, slow
              [_track(rng, 5, 0, m[3]), None, _track(rng, 5, 2, m[3])],
              [_track(rng, 10, 0, m[4]), _track(rng, 5, 2, m[4])]]
    return scenes, cfgs, dts, tracks


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_every_tick_matches_the_oracle(z_spread):
    """10 integrating ticks, every scene re-synchronised every tick against O.free_step; the geometry is the twin's at tau with the
    absent vehicles LEFT OUT of the oracle's list: v' plain 1e-5, x' 1e-6."""
    scenes, cfgs, dts, tracks = _oracle_case(z_spread)
    b = _tracked(scenes, cfgs, dts, tracks)
    try:
        assert b.planar == (z_spread == 0.0)
        empty_with_force = 0
        for t in range(10):
            _twin(scenes, tracks, t, dts if t else None)
            _check_twin(b, scenes, t, f"tick {t}")
            before, wps = b.state(), b.waypoints()
            b.tick(integrate=True)
            after = b.state()
            for k, (sc, cfg, dt) in enumerate(zip(scenes, cfgs, dts)):
                n = len(sc["loc"])
                if n == 0:
                    continue
                here = sc["dynamic_present"]
                empty_with_force += int(len(here) > 0 and not here.any())
                loc, vel = before[k]
                wp3 = np.zeros((n, 3))
                wp3[:, :2] = wps[k][0]
                prm = O.OracleParams.from_config(cfg)
                geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"],
                                  dynamic_obstacles=[v for v, p in zip(sc["dynamic_obstacles"], here) if p],
                                  dynamic_vel=sc["dynamic_vel"][here])
                crossing = np.zeros(n, bool)
                with np.errstate(all="ignore"):
                    oloc, ovel, _, _ = O.free_step(loc, vel, wp3, sc["target_speed"], sc["radius"], crossing,
                                                   wps[k][1].astype(np.int64), geom, prm, dt, arrive_threshold=2.0,
                                                   seed=0, world_side=1.0, redraw=False, round_f32=True)
                    diag = {}
                    O.tick_forces(loc, vel, wp3, sc["target_speed"], sc["radius"], crossing, geom, prm,
                                  theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
                dloc, dvel = after[k]
                P.check_velocity(dvel, ovel, diag["total"][0], dt)
                assert np.max(np.abs(dloc - oloc)) <= 1e-6 * max(1.0, np.max(np.abs(oloc))) + 1e-6, f"scene {k} tick {t}"
        assert empty_with_force >= 4                                          # scene 0 in ticks 0-2, scene 1 in tick 5
    finally:
        b.close()


def test_tracks_that_restate_free_running_change_nothing():
    """Tracks whose keyframes are advance_center_f32's centres tick after tick, with the vehicle's own velocity and yaw, and a batch
    given only empty tracks, equal the free-running batch bitwise over 8 ticks: state and vehicles."""
    scenes = [V._scene(64, 51, 4), V._scene(17, 52, 1), V._scene(0, 53, 2)]
    cfgs = [V._config(k, ALL) for k in range(3)]
    dts = [0.05, 0.04, 0.02]
    boxes = pack_boxes(scenes)
    kx, ky, kvx, kvy, kc, ks, lens = [], [], [], [], [], [], []
    for sc, dt in zip(scenes, dts):
        for j, (c, _) in enumerate(sc["dynamic_obstacles"]):
            for _ in range(9):
                kx.append(c[0]); ky.append(c[1])
                c = scenarios.advance_center_f32(c, sc["dynamic_vel"][j], dt)
            kvx += [sc["dynamic_vel"][j][0]] * 9
            kvy += [sc["dynamic_vel"][j][1]] * 9
            kc += [np.float32(np.cos(sc["dynamic_yaw"][j]))] * 9
            ks += [np.float32(np.sin(sc["dynamic_yaw"][j]))] * 9
            lens.append(9)
    packed = {"trk_off": np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), "first_tick": np.zeros(len(lens), np.int32)}
    packed.update({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in
                   zip(("kx", "ky", "kvx", "kvy", "kcos", "ksin"), (kx, ky, kvx, kvy, kc, ks))})
    assert np.array_equal(packed["kvx"][::9], boxes[8]) and np.array_equal(packed["kcos"][::9], boxes[6])   # what the boxes hold
    free, tracked, empty = (V._batch(scenes, cfgs, dts) for _ in range(3))
    try:
        tracked.set_vehicle_tracks(packed)
        empty.set_vehicle_tracks([None, [None], None])
        for t in range(8):
            for b in (free, tracked, empty):
                b.run(1)
            V._assert_same(V._everything(free), V._everything(tracked), f"restated tracks, tick {t}")
            V._assert_same(V._everything(free), V._everything(empty), f"empty tracks, tick {t}")
        assert tracked.vehicle_tracks()[0] == 8 and all(p.all() for p in empty.vehicle_tracks()[1])
    finally:
        for b in (free, tracked, empty):
            b.close()


def _mode_case(seed):
    """Two scenes of 32 with make_mode_plan; vehicle 0 drives through the crowd for 18 ticks and leaves, vehicle 1 enters at
    tick 28: ticks 18 .. 27 see no vehicle at all.  One extent per scene."""
    made = [M._scene(32, seed + k, 2) for k in range(2)]
    tracks = []
    for k, (sc, _, _) in enumerate(made):
        mid = _mid(sc)
        out = []
        for j, (first, L, yaw) in enumerate(((0, 18, 0.3 + k), (28, 20, 2.0 + k))):
            speed = np.full(L, 1.4)
            d = np.array([np.cos(yaw), np.sin(yaw)])
            xy = mid - 0.5 * L * 0.05 * 1.4 * d + np.arange(L)[:, None] * 0.05 * 1.4 * d
            out.append({"xy": np.float32(xy).astype(np.float64), "yaw": np.full(L, yaw), "speed": speed, "first_tick": first})
        tracks.append(out)
    return made, tracks


@pytest.mark.parametrize("spawns", [False, True], ids=["modes", "modes+spawns"])
def test_modes_see_the_traffic_come_and_go(spawns):
    """40 ticks: modes, targets, cursors (and v', waypoints, ghosts: _Host.check) per tick against the host loop driven by the
    oracle's gap acceptance over the twin's PRESENT vehicles; with ``spawns`` one scene also runs a spawn schedule."""
    made, tracks = _mode_case(2300)
    if spawns:
        made, tracks = made[:1], tracks[:1]
    scenes, plans = [m[0] for m in made], [m[1] for m in made]
    B = len(scenes)
    cfgs = [M._config(k) for k in range(B)]
    dts, t0, thr = [0.05, 0.04][:B], [4.0, 3.0][:B], 2.0
    b = SfmBatch(cfgs, dts)
    hosts = []
    try:
        b.upload(scenes, device_vehicles=True)
        b.set_vehicle_tracks(tracks)
        b.set_modes(plans, despawn_on_arrival=True, sim_time0=t0, arrive_thresholds=thr, scenes=scenes)
        if spawns:
            scheds = [scenarios.make_spawn_plan(scenes[0], 2350, dt=dts[0], t0=t0[0], present=0.35, horizon=1.5)]
            b.set_spawns(scheds)
        assert b.vehicle_tracks()[0] == 0                                     # set_modes / set_spawns keep the tracks
        for k in range(B):
            hs = dict(scenes[k])
            if spawns:
                h = S._SpawnHost(hs, plans[k], made[k][2], cfgs[k], dts[k], thr, True, scheds[k], np.float32(t0[k]))
                h.z3, h.clock0 = False, t0[k]
            else:
                h = M._Host(hs, plans[k], made[k][2], cfgs[k], dts[k], thr, True)
            hosts.append(h)
        ev = dict(idle_wake=0, waiting=0, checking=0, crossing=0, road_to_sidewalk=0, despawn=0, popped=0, born_later=0,
                  chain_delayed=0, newborn_checking=0, born_then_despawned=0)
        crossed_unwatched = 0
        clock = np.float32(t0)
        for t in range(40):
            _twin(scenes, tracks, t)
            _check_twin(b, scenes, t, f"tick {t}")
            state, wps = b.state(), b.waypoints()
            expect = {}
            for k, h in enumerate(hosts):
                here = scenes[k]["dynamic_present"]
                assert here.any() == (not 18 <= t < 28)
                h.sc["dynamic_vel"] = scenes[k]["dynamic_vel"][here]
                h.sc["dynamic_extent"] = scenes[k]["dynamic_extent"][here]
                veh = [v for v, p in zip(scenes[k]["dynamic_obstacles"], here) if p]
                was = ev["crossing"]
                args = (state[k][0], state[k][1], wps[k][0].astype(np.float64), veh)
                expect[k] = h.tick(*args, clock[k], ev, t) if spawns else h.tick(*args, float(clock[k]), ev)
                crossed_unwatched += (ev["crossing"] - was) * (not here.any())
            b.run(1)
            clock = (clock + np.float32(dts)).astype(np.float32)
            after, wps2, modes = b.state(), b.waypoints(), b.modes()
            for k, (v_new, wp, unsure, diag) in expect.items():
                h = hosts[k]
                m, tg, cur = (a.copy() for a in modes[k])
                loc_after = after[k][0].copy()
                if spawns:
                    born, _ = b.spawns()[k]
                    assert np.array_equal(born, h.born), f"scene {k} tick {t}: births"
                    assert (m[~h.born] == MODE_UNBORN).all(), f"scene {k} tick {t}: unborn modes"
                    m[~h.born] = M.GONE
                    for i in np.nonzero(~h.born | (m == M.GONE))[0]:
                        assert np.array_equal(loc_after[i, :2], S._parked(i)), f"scene {k} tick {t}: ghost {i}"
                        loc_after[i, :2] = M._park(i)
                h.check(k, t, loc_after, after[k][1], wps2[k][0].astype(np.float64), m, tg, cur, v_new, wp, unsure, diag)
        print(f"\ntracks + modes (spawns={spawns}): {ev}, crossed with every vehicle absent: {crossed_unwatched}")
        assert ev["waiting"] >= 1, ev                                          # somebody waited at the kerb for the traffic
        assert crossed_unwatched >= 1, ev                                      # ... and somebody crossed while nobody drove
    finally:
        b.close()


def _forms_case():
    scenes = [V._scene(64, 41, 4), V._scene(17, 42, 1), V._scene(0, 43, 2), V._scene(120, 44, 6)]
    cfgs = [V._config(k, ALL) for k in range(4)]
    dts = [0.05, 0.04, 0.02, 0.05]
    rng = np.random.default_rng(79)
    m = [_mid(sc) for sc in scenes]
    tracks = [[_track(rng, 5, 4, m[0]), _track(rng, 3, 5, m[0]), _track(rng, 2, 12, m[0]), _track(rng, 4, 4, m[0])],   # frames 0-3, 9-11: nobody
              [None], [_track(rng, 20, -2, m[2]), None],
              [_track(rng, 7, j, m[3]) for j in range(5)] + [None]]
    return scenes, cfgs, dts, tracks


def test_run_forms_agree():
    """run(16) == 16 x tick(integrate=True) == run_recorded(16) == run_recorded_forces(16) bit for bit, pedestrians and vehicles;
    the dynamic_obstacle_force record is exactly zero in the frames in which the scene's vehicles are all absent, and not
    elsewhere; tick(integrate=False) moves nothing and leaves tau alone."""
    scenes, cfgs, dts, tracks = _forms_case()
    A, B_, Cb, D = (_tracked(scenes, cfgs, dts, tracks) for _ in range(4))
    try:
        A.run(16)
        for _ in range(16):
            B_.tick(integrate=True)
        V._assert_same(V._everything(A), V._everything(B_), "run(16) vs 16 x tick")
        frames, idx, _ = Cb.run_recorded(16)
        V._assert_same(V._everything(A), V._everything(Cb), "run vs run_recorded")
        frames2, _, _, forces = D.run_recorded_forces(16)
        V._assert_same(V._everything(A), V._everything(D), "run vs run_recorded_forces")
        assert all(np.array_equal(f, g) for f, g in zip(frames, frames2))
        assert [b.vehicle_tracks()[0] for b in (A, B_, Cb, D)] == [16] * 4
        rec = forces[0]["dynamic_obstacle_force"]
        for f in range(16):
            nobody = not any(scenarios.track_present(tr, f) for tr in tracks[0])
            assert nobody == (f < 4 or 9 <= f < 12 or f >= 14)
            assert (not rec[f].any()) == nobody, f"frame {f}: dynamic force record with {'no' if nobody else 'a'} vehicle present"
        still = [(loc, c, r) for loc, _, c, r in V._everything(A)]          # (a tick without integrate still writes v')
        A.tick()
        A.tick()
        V._assert_same(still, [(loc, c, r) for loc, _, c, r in V._everything(A)], "ticks without integrate")
        assert A.vehicle_tracks()[0] == 16
    finally:
        for b in (A, B_, Cb, D):
            b.close()


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_scene_is_independent_of_the_batch(z_spread):
    """A scene alone, first of five and last of five: bitwise equal after 10 ticks (state and vehicles)."""
    scenes, cfgs, dts, tracks = _oracle_case(z_spread)
    rng = np.random.default_rng(80)
    me, cfg, dt = V._scene(64, 1800, 4, z_spread), V._config(2, ALL), 0.04
    tr = [_track(rng, 6, 0, _mid(me)), None, _track(rng, 4, 3, _mid(me)), _track(rng, 9, -3, _mid(me))]
    planar = z_spread == 0.0
    got = []
    for order in ("alone", "first", "last"):
        rest = [] if order == "alone" else list(range(4))
        sc_ = [scenes[k] for k in rest]
        lst = ([me] + sc_) if order != "last" else (sc_ + [me])
        cf = ([cfg] + [cfgs[k] for k in rest]) if order != "last" else ([cfgs[k] for k in rest] + [cfg])
        dd = ([dt] + [dts[k] for k in rest]) if order != "last" else ([dts[k] for k in rest] + [dt])
        tt = ([tr] + [tracks[k] for k in rest]) if order != "last" else ([tracks[k] for k in rest] + [tr])
        b = _tracked(lst, cf, dd, tt, planar=planar)
        try:
            b.run(10)
            got.append(V._everything(b)[-1 if order == "last" else 0])
        finally:
            b.close()
    V._assert_same([got[0]], [got[1]], "alone vs first of five")
    V._assert_same([got[0]], [got[2]], "alone vs last of five")


def _tracked_only(b, scenes, tracks, tau, what):
    """The tracked vehicles and everybody's presence against place_tracked at tau (the untracked ones went their own way)."""
    tick, present = b.vehicle_tracks()
    assert tick == tau, what
    tw = [dict(sc) for sc in scenes]
    _twin(tw, tracks, tau)
    for k, (sc, dev) in enumerate(zip(tw, b.dynamic_obstacles())):
        assert np.array_equal(present[k], sc["dynamic_present"]), f"{what}: scene {k} presence"
        for j, tr in enumerate(tracks[k] or []):
            if tr is not None:
                assert np.array_equal(dev[j][0], sc["dynamic_obstacles"][j][0]), f"{what}: scene {k} vehicle {j} centre"
                assert np.array_equal(dev[j][1], sc["dynamic_obstacles"][j][1]), f"{what}: scene {k} vehicle {j} ring"


def test_switching():
    """Tracks set twice restart tau; tracks -> set_dynamic_boxes (free running again), -> upload, ->
    sfm_batch_set_dynamic_obstacles (static rings); set_params keeps them; tracks off."""
    scenes, cfgs, dts, tracks = _forms_case()
    b = _tracked(scenes, cfgs, dts, tracks)
    ref = V._batch(scenes, cfgs, dts)
    try:
        b.run(5)
        _tracked_only(b, scenes, tracks, 5, "five ticks")
        b.set_vehicle_tracks(tracks)                              # set twice: tau restarts, placed for tau = 0 again
        _tracked_only(b, scenes, tracks, 0, "tracks set twice")
        b.run(2)
        _tracked_only(b, scenes, tracks, 2, "two ticks after the second set")
        # -> set_dynamic_boxes: the tracks go, the vehicles run free exactly as in a batch that never had any
        b.set_dynamic_boxes(scenes)
        with pytest.raises(_lib.SfmLibraryError, match="no vehicle tracks"):
            b.vehicle_tracks()
        b.run(3)
        ref.run(3)
        for k, (u, v) in enumerate(zip(b.dynamic_obstacles(), ref.dynamic_obstacles())):
            assert all(np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) for a, c in zip(u, v)), f"scene {k}"
        # -> upload drops the tracks: bit for bit the batch that never had any
        b.set_vehicle_tracks(tracks)
        b.upload(scenes, device_vehicles=True)
        ref.upload(scenes, device_vehicles=True)
        with pytest.raises(_lib.SfmLibraryError, match="no vehicle tracks"):
            b.vehicle_tracks()
        b.run(4)
        ref.run(4)
        V._assert_same(V._everything(b), V._everything(ref), "after upload")
        # -> static rings (sfm_batch_set_dynamic_obstacles): the tracks go, the rings stay where they were set
        b.set_vehicle_tracks(tracks)
        pk = pack_scenes(scenes)
        dy = pk["dynamic"]
        b._check(b._lib.sfm_batch_set_dynamic_obstacles(b._b, *(_lib.iptr(a) for a in dy[:2]), *(_lib.fptr(a) for a in dy[2:])),
                 "sfm_batch_set_dynamic_obstacles")
        with pytest.raises(_lib.SfmLibraryError, match="device-side vehicles"):
            b.set_vehicle_tracks(tracks)
        rings = b.dynamic_obstacles()
        b.run(3)
        for u, v in zip(rings, b.dynamic_obstacles()):
            assert all(np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) for a, c in zip(u, v))
        # set_params keeps the tracks and tau
        b.upload(scenes, device_vehicles=True)
        b.set_vehicle_tracks(tracks)
        b.run(2)
        b.set_params(cfgs, [0.03] * 4)
        _tracked_only(b, scenes, tracks, 2, "after set_params")
        # tracks off: the vehicles run free from where they are, an absent one stays absent
        b.set_vehicle_tracks(None)
        here = b.dynamic_obstacles()[0]
        b.run(1)
        there = b.dynamic_obstacles()[0]
        assert np.isposinf(here[0][0]).all() and np.isposinf(there[0][0]).all() and np.isposinf(there[0][1]).all()
    finally:
        b.close()
        ref.close()


def test_refusals_leave_the_batch_usable():
    scenes, cfgs, dts, tracks = _forms_case()
    b = _tracked(scenes, cfgs, dts, tracks)
    L = b._lib
    try:
        b.run(2)
        before = V._everything(b)
        pt = pack_tracks(tracks, scenes)
        T = int(pt["trk_off"][-1])

        def call(**over):
            a = dict(pt)
            a.update(over)
            ptr = lambda v, f: None if v is None else f(v)
            return L.sfm_batch_set_vehicle_tracks(b._b, ptr(a["trk_off"], _lib.iptr), ptr(a["first_tick"], _lib.iptr),
                                                  *(ptr(a[k], _lib.fptr) for k in ("kx", "ky", "kvx", "kvy", "kcos", "ksin")))

        def bad(arr, i, v):
            arr = arr.copy()
            arr[i] = v
            return arr

        cases = [(dict(trk_off=bad(pt["trk_off"], 0, 1)), "trk_off[0] must be 0"),
                 (dict(trk_off=bad(pt["trk_off"], 2, 0)), "non-decreasing"),
                 (dict(trk_off=bad(pt["trk_off"], -1, (1 << 22) + 1)), "SFM_BATCH_MAX_TRACK_KEYS"),
                 (dict(first_tick=None), "NULL"), (dict(kvy=None), "NULL"), (dict(kcos=None), "NULL"),
                 (dict(kx=bad(pt["kx"], T - 1, np.nan)), "not finite"), (dict(kvx=bad(pt["kvx"], 0, np.inf)), "not finite"),
                 (dict(ksin=bad(pt["ksin"], 3, -np.inf)), "not finite")]
        for over, why in cases:
            assert call(**over) != 0, why
            assert why in L.sfm_batch_last_error(b._b).decode(), (why, L.sfm_batch_last_error(b._b))
            V._assert_same(before, V._everything(b), f"after the refusal '{why}'")
            assert b.vehicle_tracks()[0] == 2
        # the download call: NULLs skip
        assert L.sfm_batch_download_vehicle_tracks(b._b, None, None) == 0
        with pytest.raises(ValueError, match="tracks of"):
            b.set_vehicle_tracks(pack_tracks(tracks[:1], scenes[:1]))
        b.run(1)
        assert b.vehicle_tracks()[0] == 3
        # no device-side vehicles: refused, and the batch still runs
        c = SfmBatch(cfgs, dts)
        try:
            c.upload(scenes)
            still = c.state_arrays()
            with pytest.raises(_lib.SfmLibraryError, match="device-side vehicles"):
                c.set_vehicle_tracks(tracks)
            with pytest.raises(_lib.SfmLibraryError, match="no vehicle tracks"):
                c.vehicle_tracks()
            assert all(np.array_equal(u, v) for u, v in zip(still, c.state_arrays()))
            c.run(1)
        finally:
            c.close()
    finally:
        b.close()
