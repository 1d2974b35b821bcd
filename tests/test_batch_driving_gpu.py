"""GPU tests of the batch's driven vehicles (sfm_batch_set_vehicle_driving, sfm_batch_set_vehicle_commands,
sfm_batch_download_vehicle_driving, SFM_BATCH_PTR_VEHICLE_COMMANDS; SfmBatch.set_vehicle_driving / set_vehicle_commands /
vehicle_driving / vehicle_command_tensor): the vehicles against the host twin scenarios.drive_vehicles bit for bit, the tick against
the oracle with the twin's geometry, kind 0 as a no-op on every feature form, gap acceptance seeing the command, the run forms
against each other, batch invariance, snapshot and restart, device tensors, refusals and lifetime.  Built on the recipes of
test_batch_vehicles_gpu.py and test_batch_tracks_gpu.py.  Run on the MI355X box with  python -m pytest tests -m gpu."""
import copy
from functools import lru_cache

import numpy as np
import pytest

import _driving_cases as D
import _parity as P
import test_batch_modes_gpu as M
import test_batch_steering_gpu as T
import test_batch_tracks_gpu as TR
import test_batch_vehicles_gpu as V
from carla_social_force_model_amd import observe, scenarios
from carla_social_force_model_amd._lib import SfmLibraryError
from carla_social_force_model_amd.batch import PTR_VEHICLE_COMMANDS, PTR_VEHICLE_OBS, SfmBatch, plan_from_managers
from carla_social_force_model_amd.host_state import PedMode, PedModeManager
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

ALL, NO_DYN = V.ALL, V.NO_DYN
TURN = (np.float32(np.cos(0.03)), np.float32(np.sin(0.03)))
BACK = (np.float32(np.cos(-0.05)), np.float32(np.sin(-0.05)))


def _driven(scenes, cfgs, dts, tracks, kinds, cmds, planar=None):
    b = V._batch(scenes, cfgs, dts, planar)
    try:
        if tracks is not None:
            b.set_vehicle_tracks(tracks)
        b.set_vehicle_driving(kinds, cmds)
    except Exception:
        b.close()
        raise
    D.start_twin(scenes, tracks)
    return b


def _vehicles(b):
    """Everything a tick can change about the vehicles: per scene (centres, rings, headings, velocities)."""
    drv = b.vehicle_driving()
    return [([c for c, _ in veh], [r for _, r in veh], d[2], d[3]) for veh, d in zip(b.dynamic_obstacles(), drv)]


def _check_twin(b, scenes, what):
    for k, (sc, dev, (ctr, ring, head, vel)) in enumerate(zip(scenes, b.dynamic_obstacles(), _vehicles(b))):
        V._same_vehicles(dev, sc, f"{what}: scene {k}")
        if len(dev):
            assert np.array_equal(head, sc["dynamic_heading"]), f"{what}: scene {k} headings"
            assert np.array_equal(vel, np.float32(sc["dynamic_vel"])), f"{what}: scene {k} velocities"


def _twin_case():
    return copy.deepcopy(_made_twin_case())


@lru_cache(maxsize=None)
def _made_twin_case():
    """Six scenes of 30, 20, 64, 100, 0 and 40 rows with 0, 1, 4, 6, 4 and 1 vehicles; rings of 6 and 68 points; kinds 0, 1 and 2
    mixed inside a scene; a zero command, a reverse, driven vehicles that have keyframes, a driven vehicle that is absent."""
    counts, sizes = (0, 1, 4, 6, 4, 1), (30, 20, 64, 100, 0, 40)
    scenes = [V._scene(n, 2100 + k, m, slow=False) for k, (n, m) in enumerate(zip(sizes, counts))]
    scenes[1]["dynamic_extent"] = np.array([[0.1, 0.1]])                 # a 6-point ring (the others: 68 points, two lane passes)
    V._restart_twin(scenes[1])
    assert len(scenes[1]["dynamic_obstacles"][0][1]) == 6 and len(scenes[2]["dynamic_obstacles"][0][1]) == 68
    cfgs = [V._config(k, NO_DYN if k == 2 else ALL) for k in range(6)]
    dts = [0.05, 0.04, 0.02, 0.05, 0.03, 0.05]
    rng = np.random.default_rng(91)
    m = [TR._mid(sc) for sc in scenes]
    tracks = [None,
              None,
              [TR._track(rng, 20, -3, m[2]), TR._track(rng, 12, 0, m[2]), TR._track(rng, 4, 5, m[2]), None],
              [TR._track(rng, 15, 0, m[3]), TR._track(rng, 20, -3, m[3]), None, None, TR._track(rng, 3, 2, m[3]), None],
              [None, None, TR._track(rng, 10, 5, m[4]), TR._track(rng, 8, -3, m[4])],
              None]
    kinds = [[], [1], [2, 0, 1, 1], [0, 2, 1, 2, 0, 2], [1, 2, 0, 0], [2]]
    cmds = [np.zeros((0, 3), np.float32),
            np.float32([[3.0, -4.0, 7.0]]),
            np.float32([[6.0, *TURN], [0, 0, 0], [1.0, 2.0, 0.0], [0.0, 0.0, 0.0]]),      # keyframes ignored; absent and driven; zero command
            np.float32([[0, 0, 0], [4.0, *BACK], [-2.0, 1.5, 0.0], [-3.0, *TURN], [0, 0, 0], [9.0, *TURN]]),   # a reverse
            np.float32([[0.5, 0.5, 0.0], [2.0, *TURN], [0, 0, 0], [0, 0, 0]]),
            np.float32([[1.0, 0.0, 0.0]])]                                                    # a degenerate turn: the heading stays
    return scenes, cfgs, dts, tracks, kinds, cmds


def test_vehicles_follow_the_twin():
    """Before each of 12 run(1) and after the last, every scene's centres, rings, headings and velocities equal drive_vehicles bit
    for bit; at tick 6 a driven vehicle's kind goes back to 0 and its track takes over at tau."""
    scenes, cfgs, dts, tracks, kinds, cmds = _twin_case()
    b = _driven(scenes, cfgs, dts, tracks, kinds, cmds)
    try:
        assert not np.isfinite(scenes[2]["dynamic_obstacles"][2][0]).any()    # the driven absent vehicle
        turned = 0
        for t in range(13):
            _check_twin(b, scenes, f"tick {t}")
            assert b.vehicle_tracks()[0] == t                                 # tau goes on counting
            if t == 6:
                assert np.isfinite(scenes[3]["dynamic_obstacles"][1][0]).all()
                kinds = copy.deepcopy(kinds)
                kinds[3][1] = 0
                b.set_vehicle_driving(kinds, cmds)
            if t < 12:
                h0 = [sc["dynamic_heading"].copy() for sc in scenes]
                b.run(1)
                D.drive_twin(scenes, kinds, cmds, dts, tracks, t + 1)
                turned += sum(int((a != sc["dynamic_heading"]).any(axis=1).sum()) for a, sc in zip(h0, scenes))
            if t == 6:                                                        # back on its keyframes, at tau = 7: keyframe 10
                want = np.float32(tracks[3][1]["xy"][10])
                assert np.array_equal(np.float32(scenes[3]["dynamic_obstacles"][1][0]), want)
        assert turned > 50
        assert not np.isfinite(scenes[2]["dynamic_obstacles"][2][0]).any() and not scenes[2]["dynamic_vel"][2].any()
        assert np.array_equal(scenes[5]["dynamic_heading"], scenarios.vehicle_headings({"dynamic_yaw": scenes[5]["dynamic_yaw"]}))
    finally:
        b.close()


def _oracle_kinds(scenes):
    kinds = [[1, 0, 2, 0], [2, 0], [1], [0, 2, 0], [1, 0]]
    cmds = [np.float32([[0.8, -0.5, 0.0], [0, 0, 0], [1.2, *TURN], [0, 0, 0]]), np.float32([[-0.7, *BACK], [0, 0, 0]]),
            np.float32([[0.0, 0.0, 0.0]]), np.float32([[0, 0, 0], [1.0, *TURN], [0, 0, 0]]), np.float32([[-0.3, 0.9, 0.0], [0, 0, 0]])]
    return kinds, cmds


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_every_tick_matches_the_oracle(z_spread):
    """10 integrating ticks, every scene re-synchronised every tick against O.free_step; the geometry is the twin's (absent vehicles
    left out, the velocities the commands left): v' plain 1e-5, x' 1e-6."""
    scenes, cfgs, dts, tracks = TR._oracle_case(z_spread)
    tracks[0] = None                                                          # scene 0: four free vehicles, two of them driven
    kinds, cmds = _oracle_kinds(scenes)
    b = _driven(scenes, cfgs, dts, tracks, kinds, cmds)
    try:
        assert b.planar == (z_spread == 0.0)
        for t in range(10):
            _check_twin(b, scenes, f"tick {t}")
            before, wps = b.state(), b.waypoints()
            b.tick(integrate=True)
            after = b.state()
            for k, (sc, cfg, dt) in enumerate(zip(scenes, cfgs, dts)):
                n = len(sc["loc"])
                if n == 0:
                    continue
                here = sc["dynamic_present"]
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
            D.drive_twin(scenes, kinds, cmds, dts, tracks, t + 1)
    finally:
        b.close()


def _form(feat, drive):
    """A batch of test_batch_steering_gpu's scenes in one of its feature forms, always with device-side vehicles."""
    scenes, plans, scheds, tracks = T._made(False)
    B = len(scenes)
    b = SfmBatch([M._config(k) for k in range(B)], list(T.REPLAY_DTS))
    try:
        b.upload(scenes, device_vehicles=True)
        if feat == "redraw":
            b.set_waypoint_streams([21 + k for k in range(B)], 30.0, 2.0)
        if feat in ("tracks", "spawns"):
            b.set_vehicle_tracks(tracks)
        if feat in ("modes", "spawns"):
            b.set_modes(plans, despawn_on_arrival=True, sim_time0=list(T.REPLAY_T0), arrive_thresholds=2.0, scenes=scenes)
        if feat == "spawns":
            b.set_spawns(scheds)
        if drive:
            b.set_vehicle_driving(0, np.float32([3.0, 1.0, 0.5]))        # kind 0 everywhere, commands that would matter
    except Exception:
        b.close()
        raise
    return b


@pytest.mark.parametrize("feat", ["plain", "redraw", "modes", "spawns", "tracks"])
def test_kind_zero_everywhere_is_a_no_op(feat):
    """Bit for bit against the same batch without driving, after each of 6 ticks, everything a tick writes; then kind 3 written on
    the device counts as 0 too."""
    a, b = _form(feat, False), _form(feat, True)
    try:
        import torch
        for t in range(6):
            if t == 3:
                b.set_stream(torch.cuda.current_stream().cuda_stream)
                b.vehicle_command_tensor()[:, 3] = 3.0
            a.run(1, redraw=feat == "redraw")
            b.run(1, redraw=feat == "redraw")
            T._assert_batches(T._read(b, feat), T._read(a, feat), f"{feat}, tick {t}")
        assert all(not d[0].any() for d in b.vehicle_driving())
    finally:
        a.close()
        b.close()


def test_gap_acceptance_sees_the_command():
    """A CHECKING_TRAFFIC row waits while a driven vehicle approaches; a command stops the vehicle, and the row crosses in the tick
    the oracle's gap acceptance says on the twin's vehicle."""
    dt, ts = 0.05, 1.2
    sc = D.one_vehicle_scene(c=(-12.0, 4.0), yaw=0.0, vel=(6.0, 0.0))
    sc.update(loc=np.array([[0.0, 0.0, 0.0]]), vel=np.zeros((1, 3)), waypoint=np.array([[0.0, 8.0, 0.0]]), target_speed=np.array([ts]),
              radius=np.array([0.3]), borders=[], border_centers=np.zeros((0, 2)), border_lengths=np.zeros(0), static_obstacles=[])
    mgr = PedModeManager("ped_0", ts, PedMode.WALKING_SIDEWALK, 1.5, 1.0)
    mgr.set_mode(PedMode.CROSSING_ROAD)
    assert mgr.current_mode == PedMode.CHECKING_TRAFFIC
    plan = plan_from_managers([mgr], [[(np.array([0.0, 20.0, 0.0]), False)]])
    b = SfmBatch([M._config(0)], [dt])
    try:
        b.upload([sc], device_vehicles=True)
        b.set_modes([plan], despawn_on_arrival=False, sim_time0=0.0, arrive_thresholds=0.5, scenes=[sc])
        b.set_vehicle_driving(1, np.float32([6.0, 0.0, 0.0]))
        D.start_twin([sc])
        waited, crossed_at, stop_at = 0, None, 5
        for t in range(12):
            _check_twin(b, [sc], f"tick {t}")
            loc = b.state()[0][0]
            wp = np.zeros(3)
            wp[:2] = b.waypoints()[0][0][0]
            go = O.gap_accepted(loc[0], wp, mgr.crossing_speed, mgr.crossing_safety_margin, [sc["dynamic_obstacles"][0][0]],
                                sc["dynamic_vel"], sc["dynamic_extent"])
            if t == stop_at:
                b.set_vehicle_commands(np.zeros(3, np.float32))
            b.run(1)
            D.drive_twin([sc], [1], [np.float32([0.0, 0.0, 0.0] if t >= stop_at else [6.0, 0.0, 0.0])], [dt], None, t + 1)
            mode = int(b.modes()[0][0][0])
            if crossed_at is None:
                assert (mode == int(PedMode.CROSSING_ROAD)) == bool(go), f"tick {t}: the twin says go = {go}, the device mode {mode}"
                if go:
                    crossed_at = t
                else:
                    waited += 1
                    assert mode == int(PedMode.CHECKING_TRAFFIC)
        assert crossed_at is not None and waited >= 3, (crossed_at, waited)
        assert crossed_at == stop_at + 1                                   # the stop is stored by tick stop_at, seen by the next
    finally:
        b.close()


def _small_case():
    scenes, cfgs, dts, tracks, kinds, cmds = _twin_case()
    pick = [1, 2, 3, 4]
    sub = lambda xs: [xs[k] for k in pick]
    return sub(scenes), sub(cfgs), sub(dts), sub(tracks), sub(kinds), sub(cmds)


def test_run_forms_agree():
    """run(K) == K x run(1) bit for bit; run_recorded(K) shows the same frames and leaves the same batch: the commands are held for
    all ticks, a kind 2 vehicle turning in every one."""
    K = 6
    A, B_, Cb = (_driven(*copy.deepcopy(_small_case())) for _ in range(3))
    try:
        A.run(K)
        want = [[] for _ in range(4)]
        for _ in range(K):
            for s, (loc, vel) in enumerate(B_.state()):
                want[s].append(np.float32(np.concatenate([loc[:, :2], vel[:, :2]], axis=1)))
            B_.run(1)
        V._assert_same(V._everything(A), V._everything(B_), "run(K) vs K x run(1)")
        V._assert_same(_vehicles(A), _vehicles(B_), "run(K) vs K x run(1): vehicles")
        frames, idx, _ = Cb.run_recorded(K)
        assert list(idx) == list(range(K))
        for s in range(4):
            assert np.array_equal(frames[s], np.stack(want[s]).reshape(K, -1, 4)), f"scene {s}: frames"
        V._assert_same(V._everything(Cb), V._everything(B_), "run_recorded vs K x run(1)")
        V._assert_same(_vehicles(Cb), _vehicles(B_), "run_recorded vs K x run(1): vehicles")
        h0 = scenarios.vehicle_headings(_small_case()[0][1])
        assert (A.vehicle_driving()[1][2][0] != h0[0]).any()                  # the kind 2 vehicle turned
        still = _vehicles(A)
        A.tick()                                                              # no SFM_TICK_INTEGRATE: nobody moves or turns
        V._assert_same(still, _vehicles(A), "a tick that does not integrate")
    finally:
        for b in (A, B_, Cb):
            b.close()


def test_a_scene_does_not_depend_on_the_rest_of_the_batch():
    """Scene 3 of the twin case alone and at index 2 of a batch of 4, over 8 ticks: state, vehicles and vehicle observations."""
    scenes, cfgs, dts, tracks, kinds, cmds = _small_case()
    alone = _driven(*copy.deepcopy((scenes[2:3], cfgs[2:3], dts[2:3], tracks[2:3], kinds[2:3], cmds[2:3])))
    mixed = _driven(*copy.deepcopy((scenes, cfgs, dts, tracks, kinds, cmds)))
    try:
        goals = np.float32(np.arange(12).reshape(6, 2))
        alone.set_vehicle_observation(4, 6.0, 1, goals=goals)
        mixed.set_vehicle_observation(4, [3.0, 9.0, 6.0, 2.0], 1, goals=[None, None, goals, None])
        for _ in range(2):
            alone.run(4)
            mixed.run(4)
            V._assert_same(V._everything(alone), V._everything(mixed)[2:3], "alone vs index 2")
            V._assert_same(_vehicles(alone), _vehicles(mixed)[2:3], "alone vs index 2: vehicles")
            oa, om = alone.vehicle_observations()[0], mixed.vehicle_observations()[2]
            assert oa.shape == (6, 32) and np.array_equal(oa, om, equal_nan=True) and oa[:, 6].sum() >= 5
    finally:
        alone.close()
        mixed.close()


@pytest.mark.parametrize("device", [False, True], ids=["restart", "restart_device"])
def test_snapshot_and_restart(device):
    """Snapshot, drive 7 ticks, restart scenes 1 and 3: their headings, centres, velocities, rings and rows equal the snapshot, the
    others are untouched, the commands unchanged."""
    b = _driven(*copy.deepcopy(_small_case()))
    try:
        import torch
        b.run(3)
        b.snapshot()
        snap_v, snap_s, cmd0 = _vehicles(b), V._everything(b), b.vehicle_driving()
        b.run(7)
        moved_v, moved_s = _vehicles(b), V._everything(b)
        assert any((a != c).any() for a, c in zip(snap_v[1][2], moved_v[1][2]))     # headings turned since the snapshot
        mask = np.array([0, 1, 0, 1], bool)
        if device:
            b.set_stream(torch.cuda.current_stream().cuda_stream)
            b.restart_device(torch.as_tensor(mask, device="cuda"))
        else:
            b.restart(mask)
        now_v, now_s, cmd1 = _vehicles(b), V._everything(b), b.vehicle_driving()
        for k in range(4):
            V._assert_same([now_v[k]], [snap_v[k] if mask[k] else moved_v[k]], f"scene {k}: vehicles")
            V._assert_same([now_s[k]], [snap_s[k] if mask[k] else moved_s[k]], f"scene {k}: state")
            assert np.array_equal(cmd0[k][0], cmd1[k][0]) and np.array_equal(cmd0[k][1], cmd1[k][1]), f"scene {k}: commands"
    finally:
        b.close()


def test_device_tensors():
    """torch writes vehicle_command_tensor() and reads vehicle_observation_tensor() on the batch's stream: the same as the
    host-array path (set_vehicle_commands, vehicle_observations)."""
    import torch
    case = _small_case()
    new = [np.float32(c) * np.float32(0.5) + np.float32([0.25, 0.0, 0.0]) for c in case[5]]
    a, b = (_driven(*copy.deepcopy(case)) for _ in range(2))
    try:
        for x in (a, b):
            x.set_vehicle_observation(3, 5.0, 0)
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        cmd, obs = b.vehicle_command_tensor(), b.vehicle_observation_tensor()
        assert tuple(cmd.shape) == (15, 4) and tuple(obs.shape) == (15, 28)
        assert b.device_ptr(PTR_VEHICLE_COMMANDS)[1] == 15 * 16 and b.device_ptr(PTR_VEHICLE_OBS)[1] == 15 * 28 * 4
        for step in range(3):
            a.set_vehicle_commands(new)
            cmd[:, :3] = torch.as_tensor(np.concatenate(new), device="cuda")
            a.run(2)
            b.run(2)
            b.observe_vehicles()
            got = obs.clone().cpu().numpy()
            assert np.array_equal(got, np.concatenate(a.vehicle_observations()), equal_nan=True), step
            new = [c * np.float32(-1.0) for c in new]
        V._assert_same(_vehicles(a), _vehicles(b), "tensor path vs host path")
        V._assert_same(V._everything(a), V._everything(b), "tensor path vs host path: state")
    finally:
        a.close()
        b.close()


def test_refusals_leave_the_batch_usable_and_lifetime():
    scenes, cfgs, dts, tracks, kinds, cmds = copy.deepcopy(_small_case())
    b = SfmBatch(cfgs, dts)
    try:
        b.upload(scenes)                                                      # rings that stay: no device-side vehicles
        for call in (lambda: b.set_vehicle_driving(kinds, cmds), lambda: b.set_vehicle_commands(cmds), b.vehicle_driving,
                     lambda: b.set_vehicle_observation(2, 4.0), b.observe_vehicles, b.vehicle_command_tensor,
                     b.vehicle_observation_tensor):
            with pytest.raises(SfmLibraryError):
                call()
        L, h = b._lib, b._b
        z = np.zeros(16, np.float32)
        assert L.sfm_batch_set_vehicle_driving(h, np.zeros(16, np.uint8).ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data) == -3
        assert b"sfm_batch_set_dynamic_boxes" in L.sfm_batch_last_error(h)
        b.set_dynamic_boxes(scenes)
        b.set_vehicle_tracks(tracks)
        with pytest.raises(SfmLibraryError, match="driving is off"):
            b.set_vehicle_commands(cmds)
        kd = np.zeros(15, np.uint8)
        kd[4] = 3
        bad = np.zeros(15, np.float32)
        bad[2] = np.inf
        for args in ((kd, z, z, z), (np.ones(15, np.uint8), z, None, z), (np.ones(15, np.uint8), bad, z, z)):
            rc = L.sfm_batch_set_vehicle_driving(h, args[0].ctypes.data, *(None if a is None else a.ctypes.data for a in args[1:]))
            assert rc == -1, L.sfm_batch_last_error(h)
        assert not b.driving
        with pytest.raises(SfmLibraryError, match="driving is off"):
            b.vehicle_driving()
        b.set_vehicle_driving(kinds, cmds)
        with pytest.raises(SfmLibraryError, match="not finite"):
            b.set_vehicle_commands([np.full_like(c, np.inf) for c in cmds])
        before = b.vehicle_driving()
        assert [d[0].tolist() for d in before] == kinds and all(np.array_equal(d[1], c) for d, c in zip(before, cmds))
        # every other call keeps driving and the vehicle observations
        b.set_vehicle_observation(2, 4.0)
        b.set_vehicle_tracks(None)
        b.snapshot()
        b.set_params(cfgs, dts)
        b.set_steering(0)
        b.set_observation(2, 3.0)
        b.run(2)
        b.restart()
        assert [d[0].tolist() for d in b.vehicle_driving()] == kinds and b.vehicle_observations()[1].shape == (4, 24)
        b.set_vehicle_driving(None)
        assert not b.driving
        with pytest.raises(SfmLibraryError, match="driving is off"):
            b.vehicle_command_tensor()
        b.run(1)                                                              # free running again, from where they are
        b.set_vehicle_driving(kinds, cmds)
        b.set_dynamic_boxes(scenes)                                           # new vehicles: driving and their observations go
        assert not b.driving and b.vobs_k is None
        for call in (b.vehicle_driving, b.observe_vehicles, lambda: b.set_vehicle_commands(cmds)):
            with pytest.raises(SfmLibraryError, match="off"):
                call()
        b.run(1)
    finally:
        b.close()
