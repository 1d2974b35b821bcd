"""GPU tests of the batch's vehicle autopilot (sfm_batch_set_vehicle_autopilot, sfm_batch_download_vehicle_autopilot,
sfm_batch_vehicle_autopilot_launches; SfmBatch.set_vehicle_autopilot / vehicle_autopilot): the controller against the NumPy twin
autopilot.autopilot_scene with no tolerance anywhere, then the vehicles against scenarios.drive_vehicles, scene independence, every
run path, the tick against the oracle, the behaviour the rule is for, snapshot and restart, lifetime, refusals and the launch count.
Built on the recipes of test_batch_driving_gpu.py.  Run on the MI355X box with  python -m pytest tests -m gpu."""
import copy
from functools import lru_cache

import numpy as np
import pytest

import _autopilot_cases as AC
import _driving_cases as D
import _parity as P
import test_batch_modes_gpu as M
import test_batch_steering_gpu as T
import test_batch_tracks_gpu as TR
import test_batch_vehicles_gpu as V
from carla_social_force_model_amd import autopilot as A
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd._lib import SfmLibraryError
from carla_social_force_model_amd.batch import SfmBatch
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

ALL = V.ALL
TURN = (np.float32(np.cos(0.03)), np.float32(np.sin(0.03)))
WIDE = dict(v0=6.0, T=1.0, s0=1.5, acc=1.5, dec=2.0, brake=6.0, half_width=3.0, front=1.0, look=25.0, reach=2.5, ped_margin=0.5,
            max_turn=0.04)


class Case:
    """A batch's worth of scenes with everything set_vehicle_autopilot and the twin need."""

    def __init__(self, scenes, cfgs, dts, paths, kinds, cmds, tracks=None, loop=None, ignore=None, settings=WIDE):
        self.scenes, self.cfgs, self.dts, self.paths, self.kinds, self.cmds, self.tracks = scenes, cfgs, dts, paths, kinds, cmds, tracks
        self.loop = loop if loop is not None else [[k % 2 == 0 for k in range(len(p))] for p in paths]
        self.ignore = ignore if ignore is not None else [[k % 5 == 3 for k in range(len(p))] for p in paths]
        self.settings = settings
        self.item_off = np.concatenate(([0], np.cumsum([len(sc["dynamic_obstacles"]) for sc in scenes]))).astype(np.int32)

    def pick(self, ks):
        ks = list(ks)
        g = lambda a: None if a is None else [a[k] for k in ks]
        return Case(g(self.scenes), g(self.cfgs), g(self.dts), g(self.paths), g(self.kinds), g(self.cmds), g(self.tracks), g(self.loop),
                    g(self.ignore), self.settings)

    def packed(self):
        return A.pack_settings(self.item_off, loop=[np.array(x, bool) for x in self.loop], ignore_walkers=[np.array(x, bool) for x in self.ignore],
                               **self.settings)

    def batch(self, planar=None, autopilot=True):
        b = V._batch(self.scenes, self.cfgs, self.dts, planar)
        try:
            if self.tracks is not None:
                b.set_vehicle_tracks(self.tracks)
            b.set_vehicle_driving(self.kinds, self.cmds)
            if autopilot:
                self.arm(b)
        except Exception:
            b.close()
            raise
        D.start_twin(self.scenes, self.tracks)
        return b

    def arm(self, b):
        b.set_vehicle_autopilot(self.paths, loop=[np.array(x, bool) for x in self.loop], ignore_walkers=[np.array(x, bool) for x in self.ignore],
                                **self.settings)

    def twin(self):
        return Twin(self)


class Twin:
    """The host side of a Case: commands, cursors and records per scene, advanced by autopilot_scene and drive_vehicles."""

    def __init__(self, case):
        self.c = case
        st, fl = case.packed()
        io = case.item_off
        self.st = [st[io[k]:io[k + 1]] for k in range(len(case.scenes))]
        self.fl = [fl[io[k]:io[k + 1]] for k in range(len(case.scenes))]
        self.cmd = [np.column_stack((np.float32(c).reshape(-1, 3), np.float32(k).reshape(-1, 1))).astype(np.float32) if len(k) else np.zeros((0, 4), np.float32)
                    for k, c in zip(case.kinds, case.cmds)]
        for c, paths in zip(self.cmd, case.paths):                        # (set_vehicle_autopilot: an autopiloted vehicle stands, kind 2)
            for j, p in enumerate(paths):
                if p is not None and len(p):
                    c[j] = A.STOP
        self.cur = [np.zeros(len(k), np.int32) for k in case.kinds]
        self.rec = [np.zeros((len(k), 8), np.float32) for k in case.kinds]
        self.tau = 0

    def control(self, state):
        for k, sc in enumerate(self.c.scenes):
            if len(sc["dynamic_obstacles"]):
                loc, vel = state[k]
                peds = np.column_stack((loc[:, :2], vel[:, :2])) if len(loc) else np.zeros((0, 4))
                self.cmd[k], self.cur[k], rec = A.autopilot_scene(sc, peds, self.c.paths[k], self.st[k], self.fl[k], self.cur[k], self.c.dts[k], self.cmd[k])
                on = np.array([p is not None and len(p) > 0 for p in self.c.paths[k]], bool)
                self.rec[k][on] = rec[on]

    def move(self):
        self.tau += 1
        for k, sc in enumerate(self.c.scenes):
            if len(sc["dynamic_obstacles"]):
                scenarios.drive_vehicles(sc, self.cmd[k][:, 3], self.cmd[k][:, :3], self.c.dts[k], None if self.c.tracks is None else self.c.tracks[k], self.tau)

    def tick(self, state):
        self.control(state)
        self.move()


def _vehicles(b):
    drv = b.vehicle_driving()
    return [([c for c, _ in veh], [r for _, r in veh], d[2], d[3]) for veh, d in zip(b.dynamic_obstacles(), drv)]


def _check(b, tw, what, controller=True):
    scenes = tw.c.scenes
    drv = b.vehicle_driving()
    ap = b.vehicle_autopilot()
    for k, (sc, dev) in enumerate(zip(scenes, b.dynamic_obstacles())):
        V._same_vehicles(dev, sc, f"{what}: scene {k}")
        if not len(dev):
            continue
        assert np.array_equal(drv[k][2], sc["dynamic_heading"]), f"{what}: scene {k} headings"
        assert np.array_equal(drv[k][3], np.float32(sc["dynamic_vel"])), f"{what}: scene {k} velocities"
        if controller:
            assert np.array_equal(drv[k][1], tw.cmd[k][:, :3]), f"{what}: scene {k} commands\n{drv[k][1]}\n{tw.cmd[k]}"
            assert np.array_equal(drv[k][0], np.where(np.isin(tw.cmd[k][:, 3], (1, 2)), tw.cmd[k][:, 3], 0).astype(np.uint8)), f"{what}: scene {k} kinds"
            assert np.array_equal(ap[k][0], tw.cur[k]), f"{what}: scene {k} cursors"
            assert np.array_equal(ap[k][1].view(np.uint32), tw.rec[k].view(np.uint32)), f"{what}: scene {k} records\n{ap[k][1]}\n{tw.rec[k]}"


def _mixed():
    return copy.deepcopy(_made_mixed())


@lru_cache(maxsize=None)
def _made_mixed():
    """Ten scenes.  Scenes 0 to 5 have 0, 1, 63, 64, 65 and 1024 pedestrians (the lane-stride edges -- 65 is a whole pass and a
    partial one -- and the largest scene) and EVERY ONE of them has autopiloted vehicles, 1, 4, 5, 9, 3 and 4 (more than the
    workgroup's waves; rings of 68 points, two lane passes, and in scene 8 one of 6).  Scene 6 has no vehicles, scene 9 vehicles
    none of which is autopiloted, scene 7 tracked vehicles autopiloted while absent and while present, and scene 1 an autopiloted
    vehicle beside policy-driven ones of kind 1 and kind 2 and a free one."""
    sizes, counts = (0, 1, 63, 64, 65, 1024, 30, 40, 20, 25), (1, 4, 5, 9, 3, 4, 0, 3, 2, 2)
    assert all(m > 0 for n, m in zip(sizes, counts) if n in (0, 1, 63, 64, 65, 1024))
    scenes = [V._scene(n, 4100 + k, m, slow=False) for k, (n, m) in enumerate(zip(sizes, counts))]
    scenes[8]["dynamic_extent"] = np.array([[0.1, 0.1], [2.4, 1.0]])     # a 6-point ring
    V._restart_twin(scenes[8])
    for sc in scenes:                                                    # vehicles that start along their headings
        yaw = np.asarray(sc["dynamic_yaw"], dtype=np.float64)
        sp = np.linalg.norm(sc["dynamic_vel"], axis=1) if len(yaw) else np.zeros(0)
        sc["dynamic_vel"] = np.float32(np.column_stack((sp * np.cos(yaw), sp * np.sin(yaw))).reshape(-1, 2)).astype(np.float64)
    c4, yaw4 = scenes[4]["dynamic_obstacles"][0][0], float(scenes[4]["dynamic_yaw"][0])      # the 65th row, the one of the partial
    scenes[4]["loc"][64, :2] = np.float32(c4 + 0.05 * np.array([np.cos(yaw4), np.sin(yaw4)]))  # pass, the nearest thing ahead of vehicle 0
    cfgs = [V._config(k, ALL) for k in range(10)]
    dts = [0.05, 0.04, 0.02, 0.05, 0.03, 0.05, 0.05, 0.04, 0.05, 0.04]
    rng = np.random.default_rng(97)
    mid = TR._mid(scenes[7])
    tracks = [None] * 10
    tracks[7] = [TR._track(rng, 20, 5, mid), TR._track(rng, 20, -3, mid), None]       # absent at tau 0; present
    paths = [[AC.path_near(rng, sc, k, 1 + (k + j) % 5) for k in range(len(sc["dynamic_obstacles"]))] for j, sc in enumerate(scenes)]
    paths[1] = [paths[1][0], None, None, None]                           # autopiloted, kind 1, kind 2, free
    paths[3][4] = None
    paths[9] = [None, None]                                              # vehicles, none autopiloted
    kinds = [[0] * len(sc["dynamic_obstacles"]) for sc in scenes]
    cmds = [np.zeros((len(k), 3), np.float32) for k in kinds]
    kinds[1] = [0, 1, 2, 0]
    cmds[1] = np.float32([[0, 0, 0], [0.8, -0.5, 0.0], [1.2, *TURN], [0, 0, 0]])
    kinds[9] = [2, 0]
    cmds[9] = np.float32([[1.0, *TURN], [0, 0, 0]])
    return Case(scenes, cfgs, dts, paths, kinds, cmds, tracks)


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_controller_and_vehicles_follow_the_twin(z_spread):
    """8 ticks: after each, commands, cursors and records equal the twin's bit for bit, then centres, rings, headings, velocities."""
    case = _mixed()
    if z_spread:
        rng = np.random.default_rng(5)
        for sc in case.scenes:
            sc["loc"][:, 2] = np.float32(rng.uniform(0.0, z_spread, len(sc["loc"])))
    b = case.batch(planar=not z_spread)
    tw = case.twin()
    try:
        assert b.planar == (z_spread == 0.0)
        assert not np.isfinite(case.scenes[7]["dynamic_obstacles"][0][0]).any()       # the autopiloted absent vehicle
        for k, d in enumerate(b.vehicle_driving()):                                   # before any tick: the autopiloted ones stand, kind 2
            if len(d[0]):
                assert np.array_equal(d[1], tw.cmd[k][:, :3]) and np.array_equal(d[0], tw.cmd[k][:, 3].astype(np.uint8)), k
        led, rows = set(), set()
        for t in range(8):
            state = b.state()
            b.tick(integrate=True)
            tw.tick(state)
            _check(b, tw, f"tick {t}")
            led |= {int(r[1]) for rec in tw.rec for r in rec}
            rows |= {int(r[2]) for r in tw.rec[4] if r[1] == 1}
        assert led >= {0, 1, 2, 3}, led                                              # every kind of leader was met
        assert len(tw.rec[4]) == 3 and len(case.scenes[4]["loc"]) == 65 and 64 in rows   # the 65-row scene: its last row leads
        assert np.array_equal(tw.cmd[7][0], A.STOP) and not tw.rec[7][0].any()
        assert np.array_equal(tw.cmd[1][1:], np.float32([[0.8, -0.5, 0.0, 1], [1.2, *TURN, 2], [0, 0, 0, 0]]))
    finally:
        b.close()


def test_the_others_move_as_without_the_autopilot():
    """Scene 1's policy-driven and free vehicles and scene 9's: commands and motion bitwise those of the same batch without it."""
    case = _mixed().pick([1, 9, 3])
    a, b = case.batch(autopilot=False), _mixed().pick([1, 9, 3]).batch()     # (scenes of its own: batch() starts the twin in them)
    try:
        for t in range(6):
            a.run(1)
            b.run(1)
            va, vb, da, db = _vehicles(a), _vehicles(b), a.vehicle_driving(), b.vehicle_driving()
            for k, paths in enumerate(case.paths):
                for j, p in enumerate(paths):
                    if p is None:
                        for q in range(4):
                            assert np.array_equal(va[k][q][j], vb[k][q][j]), (t, k, j, q)
                        assert np.array_equal(da[k][1][j], db[k][1][j]) and da[k][0][j] == db[k][0][j]
    finally:
        a.close()
        b.close()


def test_scene_is_independent_of_the_batch():
    """Each scene alone in a batch of one reads back the bits it has inside the mixed batch, and at another position in it."""
    case = _mixed()
    order = [5, 3, 8, 0, 9, 7, 2, 1, 6, 4]
    full, moved = case.batch(), _mixed().pick(order).batch()
    try:
        full.run(5)
        moved.run(5)
        ref = (_vehicles(full), full.vehicle_driving(), full.vehicle_autopilot())
        got = (_vehicles(moved), moved.vehicle_driving(), moved.vehicle_autopilot())
        for k in (0, 1, 2, 3, 4, 5, 7, 8, 9):                            # every scene that has vehicles
            one = _mixed().pick([k]).batch()
            try:
                one.run(5)
                alone = (_vehicles(one), one.vehicle_driving(), one.vehicle_autopilot())
            finally:
                one.close()
            for what, r, g, s in zip(("vehicles", "driving", "autopilot"), ref, got, alone):
                for q in range(len(r[k])):
                    x, y, z = r[k][q], g[order.index(k)][q], s[0][q]
                    same = lambda u, v: all(np.array_equal(i, j) for i, j in zip(u, v)) if isinstance(u, list) else np.array_equal(u, v)
                    assert same(x, y) and same(x, z), (what, k, q)
    finally:
        full.close()
        moved.close()


@pytest.mark.parametrize("form", ["tick", "run", "run_recorded", "run_recorded_forces"])
def test_every_run_path_launches_the_controller(form):
    """K = 5 ticks by each run path give the vehicles, commands, cursors and records of K step-wise ticks with the twin; a tick
    without the integrate flag changes no command, cursor or record and launches no controller."""
    case = _mixed().pick([1, 2, 3, 7])
    b = case.batch()
    tw = case.twin()
    try:
        for _ in range(5):                                               # the twin needs the pedestrians tick by tick: a second batch
            state = b.state()
            b.run(1)
            tw.tick(state)
        before = (b.vehicle_driving(), b.vehicle_autopilot(), b.vehicle_autopilot_launches())
        assert before[2] == 5
        b.tick(integrate=False)
        after = (b.vehicle_driving(), b.vehicle_autopilot(), b.vehicle_autopilot_launches())
        assert after[2] == 5
        for x, y in zip(before[:2], after[:2]):
            assert all(np.array_equal(i, j) for u, v in zip(x, y) for i, j in zip(u, v))
        c = _mixed().pick([1, 2, 3, 7]).batch()
        try:
            if form == "tick":
                for _ in range(5):
                    c.tick(integrate=True)
            elif form == "run":
                c.run(5)
            elif form == "run_recorded":
                c.run_recorded(5)
            else:
                c.run_recorded_forces(5)
            assert c.vehicle_autopilot_launches() == 5
            _check(c, tw, form)
        finally:
            c.close()
    finally:
        b.close()


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_every_tick_matches_the_oracle(z_spread):
    """8 integrating ticks with autopiloted vehicles moving, every scene re-synchronised every tick against O.free_step with the
    twin's geometry: v' plain 1e-5, x' 1e-6, as the driving tests."""
    scenes, cfgs, dts, _ = TR._oracle_case(z_spread)
    rng = np.random.default_rng(12)
    paths = [[AC.path_near(rng, sc, k, 3) for k in range(len(sc["dynamic_obstacles"]))] for sc in scenes]
    kinds = [[0] * len(sc["dynamic_obstacles"]) for sc in scenes]
    cmds = [np.zeros((len(k), 3), np.float32) for k in kinds]
    slow = dict(WIDE, v0=1.2)                                            # slow vehicles: the plain bound on v' holds
    case = Case(scenes, cfgs, dts, paths, kinds, cmds, None, settings=slow)
    b = case.batch()
    tw = case.twin()
    try:
        assert b.planar == (z_spread == 0.0)
        for t in range(8):
            before, wps = b.state(), b.waypoints()
            tw.control(before)
            b.tick(integrate=True)
            after = b.state()
            for k, (sc, cfg, dt) in enumerate(zip(scenes, cfgs, dts)):
                n = len(sc["loc"])
                if n == 0:
                    continue
                loc, vel = before[k]
                wp3 = np.zeros((n, 3))
                wp3[:, :2] = wps[k][0]
                prm = O.OracleParams.from_config(cfg)
                geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"],
                                  dynamic_obstacles=list(sc["dynamic_obstacles"]), dynamic_vel=sc["dynamic_vel"])
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
            tw.move()
            _check(b, tw, f"tick {t}")
    finally:
        b.close()


def _forms_batch(feat):
    """test_batch_steering_gpu's scenes with modes and a spawn schedule (unborn and despawned rows), vehicles on the device."""
    scenes, plans, scheds, tracks = T._made(False)
    scenes = copy.deepcopy(scenes)
    B = len(scenes)
    b = SfmBatch([M._config(k) for k in range(B)], list(T.REPLAY_DTS))
    try:
        b.upload(scenes, device_vehicles=True)
        b.set_modes(plans, despawn_on_arrival=True, sim_time0=list(T.REPLAY_T0), arrive_thresholds=2.0, scenes=scenes)
        if feat == "spawns":
            b.set_spawns(scheds)
    except Exception:
        b.close()
        raise
    return b, scenes


@pytest.mark.parametrize("feat", ["modes", "spawns"])
def test_unborn_and_despawned_rows_are_never_leaders(feat):
    """With modes and a spawn schedule: 8 ticks against the twin fed with the state the batch holds, and no record names a row that
    is despawned (255) or unborn (254)."""
    b, scenes = _forms_batch(feat)
    try:
        rng = np.random.default_rng(3)
        paths = [[AC.path_near(rng, sc, k, 3) for k in range(len(sc["dynamic_obstacles"]))] for sc in scenes]
        kinds = [[0] * len(sc["dynamic_obstacles"]) for sc in scenes]
        case = Case(scenes, None, list(T.REPLAY_DTS), paths, kinds, [np.zeros((len(k), 3), np.float32) for k in kinds], None)
        D.start_twin(scenes)
        case.arm(b)
        tw = case.twin()
        dead = 0
        for t in range(8):
            state, modes = b.state(), b.modes()
            b.tick(integrate=True)
            tw.tick(state)
            _check(b, tw, f"{feat} tick {t}")
            for k, rec in enumerate(tw.rec):
                dead += int(np.isin(modes[k][0], (254, 255)).sum())
                for r in rec:
                    if r[1] == 1:
                        assert modes[k][0][int(r[2])] not in (254, 255), (t, k, r)
        assert dead > 0                                                  # there were such rows to leave out
    finally:
        b.close()


def _behaviour_batch(sc, paths, autopilot=True, free_speed=None):
    from carla_social_force_model_amd.config import default_sfm_config
    sc = copy.deepcopy(sc)
    if free_speed is not None:
        sc["dynamic_vel"] = np.array([[free_speed, 0.0]])
    b = SfmBatch([default_sfm_config(("acceleration_force",))], [0.05])
    try:
        b.upload([sc], device_vehicles=True)
        if autopilot:
            b.set_vehicle_autopilot(paths, **AC.CALM)
        b.set_vehicle_observation(1, 50.0)
    except Exception:
        b.close()
        raise
    return b


def test_a_standing_pedestrian_stops_the_vehicle_on_the_device():
    """The standing-pedestrian case of the host tests on the device: with the autopilot the ring-to-pedestrian clear_d2 of
    observe_vehicles() stays above (s0 + ped_margin - bound)^2 and the vehicle stops; the same vehicle free-running at v0 drives
    through the pedestrian (clear_d2 below the body radius squared)."""
    sc, paths = AC.standing_pedestrian()
    sc["waypoint"] = sc["loc"].copy()                                    # the pedestrian stands
    st, _ = A.pack_settings(np.array([0, 1]), **AC.CALM)
    a, b = _behaviour_batch(sc, paths), _behaviour_batch(sc, paths, False, free_speed=AC.CALM["v0"])
    try:
        low_a, low_b, s_e = np.inf, np.inf, None
        for t in range(400):
            a.run(1)
            b.run(1)
            low_a = min(low_a, float(a.vehicle_observations()[0][0, 8]))
            low_b = min(low_b, float(b.vehicle_observations()[0][0, 8]))
            rec = a.vehicle_autopilot()[0][1][0]
            if s_e is None and rec[1] == 1 and rec[3] <= st[0, 2]:
                s_e = float(rec[6])
        assert rec[6] <= AC.STOPPED * st[0, 0] and rec[1] == 1            # stopped, behind the pedestrian
        # the ring's foremost point is front' = sqrt(2) * 2.4 ahead of the centre (>= the settings' front), so the ring-to-pedestrian
        # distance is at least gap + ped_margin - (front' - front) in x
        room = st[0, 2] + st[0, 10] - (np.sqrt(2.0) * 2.4 - st[0, 7]) - AC.undershoot_bound(s_e or 0.0, st[0], 0.05)
        assert room > 0.3 and low_a >= room ** 2, (low_a, room)
        assert low_b < 0.3 ** 2, low_b
    finally:
        a.close()
        b.close()


def test_a_closed_path_is_driven_round_on_the_device():
    """The closed path of 8 points on the device, 40 calls of run(10): after each the cursor and the record are the twin's, the
    cursor visits the points in order (at most two per 10 ticks), and two laps complete within the 400 ticks."""
    sc, paths = AC.closed_path()
    st, fl = A.pack_settings(np.array([0, 1]), loop=True, **dict(AC.CALM, v0=8.0))
    recs, curs, _ = AC.run_twin(copy.deepcopy(sc), paths[0], st, fl, 0.05, 400)
    from carla_social_force_model_amd.config import default_sfm_config
    b = SfmBatch([default_sfm_config(("acceleration_force",))], [0.05])
    try:
        b.upload([copy.deepcopy(sc)], device_vehicles=True)
        b.set_vehicle_autopilot(paths, loop=True, **dict(AC.CALM, v0=8.0))
        seen = []
        for t in range(40):
            b.run(10)
            cur, rec = b.vehicle_autopilot()[0]
            assert cur[0] == curs[10 * t + 9, 0] and np.array_equal(rec[0], recs[10 * t + 9, 0]), t
            seen.append(int(cur[0]))
        steps = np.diff(np.array(seen))
        assert set(np.mod(steps, 8)) <= {0, 1, 2} and int(np.sum(np.mod(steps, 8))) >= 16      # in order, two laps
    finally:
        b.close()


def _restart_case():
    return _mixed().pick([1, 2, 3, 7])


@pytest.mark.parametrize("how", ["list", "mask", "auto"])
def test_restart_puts_the_cursors_back(how):
    """snapshot, 20 ticks, restart of scenes 0 and 2: their cursors and vehicles are the snapshot's bit for bit, scenes 1 and 3 are
    untouched, and the next 5 ticks equal those of a batch that never ran the 20 (chosen scenes) or never restarted (the others)."""
    import torch
    case = _restart_case()
    b, fresh, cont = case.batch(), _restart_case().batch(), _restart_case().batch()
    try:
        for x in (b, fresh, cont):
            x.run(3)
        b.snapshot()
        snap = (_vehicles(b), b.vehicle_autopilot())
        b.run(20)
        cont.run(20)
        moved = b.vehicle_autopilot()
        assert any((m[0] != s[0]).any() for m, s in zip(moved, snap[1]))             # cursors did move
        chosen = [0, 2]
        if how == "list":
            b.restart(chosen)
        elif how == "mask":
            b.set_stream(torch.cuda.current_stream().cuda_stream)
            mask = torch.zeros(4, dtype=torch.uint8, device="cuda")
            mask[chosen] = 1
            b.restart_device(mask)
            torch.cuda.synchronize()
        else:
            b.set_episodes(agent=[0, -1, 0, -1], max_steps=[1, 0, 1, 0])             # scenes 0 and 2 time out at once
            b.end_step(auto_restart=True)
            assert list(np.flatnonzero(b.episodes()[1])) == chosen
        veh, ap = _vehicles(b), b.vehicle_autopilot()
        cveh, cap = _vehicles(cont), cont.vehicle_autopilot()
        for k in range(4):
            rv, ra = (snap[0][k], snap[1][k]) if k in chosen else (cveh[k], cap[k])
            assert np.array_equal(ap[k][0], ra[0]), (how, k, "cursor")
            for q in range(4):
                assert all(np.array_equal(i, j) for i, j in zip(veh[k][q], rv[q])), (how, k, q)
            if k not in chosen:
                assert np.array_equal(ap[k][1], ra[1])
        for t in range(5):
            for x in (b, fresh, cont):
                x.run(1)
            veh, ap, dr = _vehicles(b), b.vehicle_autopilot(), b.vehicle_driving()
            refs = {id(r): (_vehicles(r), r.vehicle_autopilot(), r.vehicle_driving()) for r in (fresh, cont)}
            for k in range(4):
                rveh, rap, rdr = refs[id(fresh if k in chosen else cont)]
                assert np.array_equal(ap[k][0], rap[k][0]) and np.array_equal(ap[k][1], rap[k][1]), (how, t, k)
                assert np.array_equal(dr[k][1], rdr[k][1]), (how, t, k)
                for q in range(4):
                    assert all(np.array_equal(i, j) for i, j in zip(veh[k][q], rveh[k][q])), (how, t, k, q)
    finally:
        for x in (b, fresh, cont):
            x.close()


def test_restart_noise_leaves_an_autopiloted_vehicle_at_its_snapshot_pose():
    case = _restart_case()
    b = case.batch()
    try:
        b.run(3)
        b.set_restart_noise([5, 6, 7, 8], pos_box=np.array([0.5, 0.5]), track_delay=3)
        b.snapshot()
        snap, cur = _vehicles(b), [c[0] for c in b.vehicle_autopilot()]
        b.run(10)
        b.restart()
        veh = _vehicles(b)
        for k in range(4):
            for q in range(4):
                assert all(np.array_equal(i, j) for i, j in zip(veh[k][q], snap[k][q])), (k, q)
        assert all(np.array_equal(c[0], s) for c, s in zip(b.vehicle_autopilot(), cur))
        assert b.restart_noise()[0].sum() == 4                             # (the noise did run: one restart per scene)
    finally:
        b.close()


def test_restart_noise_before_the_first_tick():
    """An autopiloted vehicle counts as driven from set_vehicle_autopilot on: a restart with traffic-timing noise before any
    integrating tick leaves the tracked autopiloted vehicles, present and absent, at their snapshot pose, whatever the seed."""
    case = _mixed().pick([7, 2])
    b = case.batch()
    try:
        b.set_restart_noise([11, 12], pos_box=np.array([0.5, 0.5]), track_delay=3)
        b.snapshot()
        snap = _vehicles(b)
        assert [int(k) for k in b.vehicle_driving()[0][0]] == [2, 2, 2]
        for seed in range(4):
            b.set_restart_noise([seed, seed + 7], pos_box=np.array([0.5, 0.5]), track_delay=3)
            b.restart()
            veh = _vehicles(b)
            for k in range(2):
                for q in range(4):
                    assert all(np.array_equal(i, j) for i, j in zip(veh[k][q], snap[k][q])), (seed, k, q)
        assert b.vehicle_autopilot_launches() == 0
    finally:
        b.close()


def _off(b):
    with pytest.raises(SfmLibraryError, match="autopilot is off"):
        b.vehicle_autopilot()
    assert b.vehicle_autopilot_launches() == 0 and not b.autopilot


def test_lifetime_follows_the_driving():
    """Every drop rule: set_vehicle_driving (on or off), set_dynamic_boxes, upload; paths=None keeps the driving; a batch reused for
    another generation reads back what a fresh one does."""
    case = _mixed().pick([1, 2])
    b = case.batch(autopilot=False)
    try:
        _off(b)
        b.run(2)                                                         # (a batch that never set it: no controller launch)
        assert b.vehicle_autopilot_launches() == 0
        case.arm(b)
        assert b.autopilot and b.driving and not b.has_snapshot
        b.run(2)
        assert b.vehicle_autopilot_launches() == 2
        b.set_vehicle_driving(case.kinds, case.cmds)
        _off(b)
        case.arm(b)
        b.set_vehicle_driving(None)
        _off(b)
        with pytest.raises(SfmLibraryError, match="driving is off"):
            b.vehicle_driving()
        case.arm(b)                                                      # switches the driving on: kind 0, the autopiloted ones stand
        for d, paths in zip(b.vehicle_driving(), case.paths):
            want = np.array([A.STOP if p is not None else np.zeros(4, np.float32) for p in paths])
            assert b.driving and np.array_equal(d[0], want[:, 3].astype(np.uint8)) and np.array_equal(d[1], want[:, :3])
        b.set_vehicle_autopilot(None)
        _off(b)
        assert b.driving and len(b.vehicle_driving()) == 2
        case.arm(b)
        b.set_dynamic_boxes(case.scenes)
        _off(b)
        case.arm(b)
        b.upload(case.scenes, device_vehicles=True)
        _off(b)
        # another generation in the same batch against a fresh one
        gen = _mixed().pick([3, 8])
        b.set_params(gen.cfgs, gen.dts)
        b.upload(copy.deepcopy(gen.scenes), device_vehicles=True)
        b.set_vehicle_driving(gen.kinds, gen.cmds)
        gen.arm(b)
        f = gen.batch()
        try:
            b.run(6)
            f.run(6)
            for x, y in zip((_vehicles(b), b.vehicle_driving(), b.vehicle_autopilot()), (_vehicles(f), f.vehicle_driving(), f.vehicle_autopilot())):
                for u, v in zip(x, y):
                    for i, j in zip(u, v):
                        assert all(np.array_equal(p, q) for p, q in zip(i, j)) if isinstance(i, list) else np.array_equal(i, j)
        finally:
            f.close()
    finally:
        b.close()


def test_refused_calls_change_nothing():
    """Each refused call leaves every download and the next tick unchanged; before the upload and without device-side vehicles the
    call is refused as a state error."""
    import ctypes as C
    from carla_social_force_model_amd._lib import fptr, iptr, u8ptr
    case = _mixed().pick([1, 2])
    b, ref = case.batch(), _mixed().pick([1, 2]).batch()
    try:
        b.run(2)
        ref.run(2)
        io = case.item_off
        off, px, py = A.pack_paths(case.paths, io)
        st, fl = case.packed()
        L = b._lib

        def call(off=off, px=px, py=py, st=st, fl=fl):
            return L.sfm_batch_set_vehicle_autopilot(b._b, iptr(off), fptr(px), fptr(py), fptr(st), u8ptr(fl))

        def bad_setting(col, v):
            s = st.copy()
            s[2, col] = v
            return s
        o1 = off.copy(); o1[0] = 1
        o2 = off.copy(); o2[2] = o2[1] - 1 if o2[1] > 0 else -1
        pnan = px.copy(); pnan[0] = np.nan
        big = np.zeros(len(off), np.int32); big[1:] = A.MAX_POINTS + 1
        bigp = np.zeros(A.MAX_POINTS + 1, np.float32)
        f3 = fl.copy(); f3[0] = 4
        refused = [call(off=o1), call(off=o2), call(px=pnan), call(off=big, px=bigp, py=bigp), call(fl=f3),
                   call(st=bad_setting(0, 0.0)), call(st=bad_setting(1, -1.0)), call(st=bad_setting(2, 0.0)), call(st=bad_setting(3, np.inf)),
                   call(st=bad_setting(4, 0.0)), call(st=bad_setting(5, st[2, 4] * 0.5)), call(st=bad_setting(6, -0.1)),
                   call(st=bad_setting(7, np.nan)), call(st=bad_setting(8, 0.0)), call(st=bad_setting(9, 0.0)), call(st=bad_setting(9, 3e38)),
                   call(st=bad_setting(10, -1.0)), call(st=bad_setting(11, 0.0)), call(st=bad_setting(11, 1.5)), call(st=bad_setting(12, -0.5)),
                   L.sfm_batch_set_vehicle_autopilot(b._b, iptr(off), fptr(px), fptr(py), None, u8ptr(fl))]
        assert all(rc != 0 for rc in refused), refused
        assert b.vehicle_autopilot_launches() == 2
        for x, y in zip((_vehicles(b), b.vehicle_driving(), b.vehicle_autopilot()), (_vehicles(ref), ref.vehicle_driving(), ref.vehicle_autopilot())):
            for u, v in zip(x, y):
                for i, j in zip(u, v):
                    assert all(np.array_equal(p, q) for p, q in zip(i, j)) if isinstance(i, list) else np.array_equal(i, j)
        b.run(1)
        ref.run(1)
        for u, v in zip(b.vehicle_autopilot(), ref.vehicle_autopilot()):
            assert np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1])
        with pytest.raises(ValueError):
            b.set_vehicle_autopilot(case.paths, v0=0.0)
        with pytest.raises(ValueError):
            b.set_vehicle_autopilot(case.paths[:1])
    finally:
        b.close()
        ref.close()
    n = SfmBatch([V._config(0, ALL)], [0.05])
    try:
        with pytest.raises(SfmLibraryError):
            n.set_vehicle_autopilot([[]])
        n.upload([V._scene(5, 1, 1)])                                    # rings that stay: no device-side vehicles
        with pytest.raises(SfmLibraryError, match="device-side vehicles"):
            n.set_vehicle_autopilot([[np.array([[1.0, 2.0]])]])
        rc = n._lib.sfm_batch_set_vehicle_autopilot(n._b, iptr(np.zeros(2, np.int32)), None, None, fptr(np.ones(13, np.float32)),
                                                    u8ptr(np.zeros(1, np.uint8)))
        assert rc == -3 or rc != 0
    finally:
        n.close()


def test_the_example_runs():
    import test_batch_autopilot_host as H
    episodes, arrivals, behind_ped, behind_car = H._example().run(B=8, steps=6, repeat=2, quiet=True)
    assert episodes >= 0 and arrivals <= episodes and behind_ped + behind_car >= 0
