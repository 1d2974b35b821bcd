"""GPU tests of steered pedestrians in a batch (sfm_batch_set_steering, sfm_batch_set_commands, sfm_batch_download_steering,
sfm_batch_device_ptr; SfmBatch.set_steering / set_commands / steering / command_tensor / state_tensor).

Kind 1 rows take their command as v' bit for bit, kind 2 rows take it as the preferred velocity of the acceleration term, and
everyone else sees them as ordinary pedestrians: v' against the oracle (plain 1e-5; the conditioned bound of
test_batch_gpu.test_every_scene_matches_the_oracle for the scenes with vehicles).  Everything else is bitwise: replaying an
unsteered batch's own velocities as commands is the identity, steering that steers nobody is a no-op, a command written through the
device tensor does what set_commands does.  Scenes of 0 .. 300 pedestrians: the 4-, 2- and 1-slice j splits, the second row pass
above 256, an empty scene.  Run on the MI355X box with  python -m pytest tests -m gpu."""
from functools import lru_cache

import numpy as np
import pytest

import _parity as P
import test_batch_gpu as G
import test_batch_modes_gpu as M
import test_batch_restart_gpu as R
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import PTR_COMMANDS, PTR_STATE, PTR_ZSTATE, SfmBatch, pack_steering
from carla_social_force_model_amd._lib import SfmLibraryError
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 3, 17, 64, 65, 128, 129, 256, 257, 300)
UNSTEERED, ALL_STEERED = SIZES.index(64), SIZES.index(65)     # a scene with no steered row, a scene that is entirely steered
FORCE_SETS = (G.GEO, ("acceleration_force", "pedestrian_force"), ("pedestrian_force", "border_force", "static_obstacle_force"),
              ("acceleration_force", "border_force"))
SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3
f32 = lambda a: np.float32(a).astype(np.float64)


@lru_cache(maxsize=None)
def _setup(z_spread):
    """Scenes, configs, step lengths, kinds and commands (built once; nobody changes them).  Every scene its own parameters and dt;
    kinds from a seeded draw; two more scenes with vehicles."""
    scenes, cfgs, dts = [], [], []
    for k, n in enumerate(SIZES):
        forces = FORCE_SETS[k % len(FORCE_SETS)]
        scenes.append(G._scene(n, 700 + k, z_spread, geo="border_force" in forces, crossing=k % 3 == 0))
        cfgs.append(G._config(k, forces))
        dts.append([0.05, 0.04, 0.02][k % 3])
    dyn_first = len(scenes)
    for k, n in enumerate((40, 300)):
        scenes.append(G._scene(n, 800 + k, z_spread, dynamic=3))
        cfgs.append(G._config(k, scenarios.ALL_FORCES))
        dts.append(0.05)
    rng = np.random.default_rng(99)
    kinds, cmds = [], []
    for k, sc in enumerate(scenes):
        n = len(sc["loc"])
        kd = rng.integers(0, 3, n)
        if k == UNSTEERED:
            kd[:] = 0
        if k == ALL_STEERED:
            kd = 1 + rng.integers(0, 2, n)
        kinds.append(kd)
        cmds.append(np.float32(rng.uniform(-1.5, 1.5, (n, 3))))
    return scenes, cfgs, dts, kinds, cmds, dyn_first


def _one_tick(z_spread, steer, scenes=None, pick=None):
    """tick_forces(integrate=True) of the batch (or of its scenes ``pick``), then one more tick without integration:
    (forces, state after tick 1, state after tick 2, planar)."""
    all_scenes, cfgs, dts, kinds, cmds, _ = _setup(z_spread)
    scenes = all_scenes if scenes is None else scenes
    idx = list(range(len(scenes))) if pick is None else list(pick)
    b = SfmBatch([cfgs[k] for k in idx], [dts[k] for k in idx])
    try:
        b.upload([scenes[k] for k in idx])
        if steer:
            b.set_steering([kinds[k] for k in idx], [cmds[k] for k in idx])
        forces = b.tick_forces(integrate=True)
        first = b.state()
        b.tick()
        return forces, first, b.state(), b.planar
    finally:
        b.close()


@lru_cache(maxsize=None)
def _steered(z_spread):
    return _one_tick(z_spread, True)


@lru_cache(maxsize=None)
def _plain(z_spread):
    return _one_tick(z_spread, False)


def _oracle_forces(sc, cfg):
    n = len(sc["loc"])
    prm = O.OracleParams.from_config(cfg)
    geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"], sc["dynamic_obstacles"],
                      sc["dynamic_vel"])
    crossing = sc.get("crossing")
    crossing = np.zeros(n, bool) if crossing is None else crossing
    diag = {}
    with np.errstate(all="ignore"):
        forces, total, _ = O.tick_forces(sc["loc"], sc["vel"], sc["waypoint"], sc["target_speed"], sc["radius"], crossing, geom, prm,
                                         theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
    summed = sum(np.nan_to_num(ab) for name, (_, ab) in diag.items() if name != "total")
    return prm, forces, total, diag["total"][0], summed


def _steered_reference(sc, cfg, dt, kd, u):
    """(v' of the oracle with the acceleration row of the kind 2 rows replaced by (u - v) / tau in float64, that replaced term,
    exposure, summed term magnitudes)."""
    prm, forces, total, expo, summed = _oracle_forces(sc, cfg)
    repl = (u - sc["vel"]) / prm.tau
    k2 = kd == 2
    if "acceleration_force" in forces:
        total = total.copy()
        total[k2] += repl[k2] - forces["acceleration_force"][k2]
    return O.new_velocities(sc["vel"], total, sc["target_speed"], dt, prm.max_speed_factor), repl, expo, summed


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_velocity_and_preferred_velocity_rows(z_spread):
    """One integrating tick of the mixed batch.  Kind 1: v' is the command bitwise, x' = fp32(dt u + x) in the arithmetic of
    scenarios.advance_center_f32, and the row's force records are those of the unsteered batch bitwise.  Kind 0 and kind 2 rows:
    v' against the oracle (kind 2 with its acceleration row replaced); the acceleration slot of a kind 2 row's force record is
    the replaced term; where the acceleration force is off, kind 2 changes nothing bitwise."""
    scenes, cfgs, dts, kinds, cmds, dyn_first = _setup(z_spread)
    forces, states, _, planar = _steered(z_spread)
    pforces, pstates, _, _ = _plain(z_spread)
    assert planar == (z_spread == 0.0)
    C = 2 if planar else 3
    seen = {1: 0, 2: 0, "off": 0}
    for k, (sc, cfg, dt, kd, cmd) in enumerate(zip(scenes, cfgs, dts, kinds, cmds)):
        n = len(sc["loc"])
        if n == 0:
            continue
        loc, vel = states[k]
        u = cmd.astype(np.float64)
        if planar:
            u[:, 2] = 0.0
        k1, k2 = kd == 1, kd == 2
        assert np.array_equal(vel[k1], u[k1]), f"scene {k}: a velocity row's v' is not its command"
        x_ref = scenarios.advance_center_f32(f32(sc["loc"]), u, dt)
        assert np.array_equal(loc[k1][:, :C], x_ref[k1][:, :C]), f"scene {k}: a velocity row's x'"
        v_ref, repl, expo, summed = _steered_reference(sc, cfg, dt, kd, u)
        rest = ~k1
        if k >= dyn_first:
            needed = P.check_velocity_conditioned(vel[rest], v_ref[rest], expo[rest], summed[rest], dt)
            assert needed <= max(2, n // 100), f"scene {k}"
        else:
            P.check_velocity(vel[rest], v_ref[rest], expo[rest], dt)
        acc_on = bool(O.OracleParams.from_config(cfg).enabled["acceleration_force"])
        for name in forces[k]:
            same = ~k2 if name in ("acceleration_force", "total") and acc_on else np.ones(n, bool)
            assert np.array_equal(forces[k][name][same], pforces[k][name][same]), f"scene {k}: {name} of rows that keep their forces"
        if acc_on and k2.any():
            mag = (np.linalg.norm(u, axis=1) + np.linalg.norm(sc["vel"], axis=1)) / O.OracleParams.from_config(cfg).tau
            P.check_force("replaced acceleration term", forces[k]["acceleration_force"][k2], repl[k2][:, :C], mag[k2], np.zeros(k2.sum()))
            assert not np.array_equal(forces[k]["acceleration_force"][k2], pforces[k]["acceleration_force"][k2])
        if not acc_on:
            assert np.array_equal(vel[k2], pstates[k][1][k2]) and np.array_equal(loc[k2], pstates[k][0][k2]), f"scene {k}"
            seen["off"] += int(k2.sum())
        seen[1] += int(k1.sum())
        seen[2] += int((k2 & acc_on).sum())
    assert min(seen.values()) > 10, seen
    assert not kinds[UNSTEERED].any() and kinds[ALL_STEERED].all()


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_others_feel_the_steered_rows(z_spread):
    """The second tick starts from the state the commands produced: its unsteered rows' v' against the oracle evaluated at the
    downloaded state."""
    scenes, cfgs, dts, kinds, cmds, dyn_first = _setup(z_spread)
    _, first, second, _ = _steered(z_spread)
    for k, (sc, cfg, dt, kd) in enumerate(zip(scenes, cfgs, dts, kinds)):
        n = len(sc["loc"])
        free = kd == 0
        if n == 0 or not free.any():
            continue
        at = dict(sc, loc=first[k][0], vel=first[k][1])
        v_ref, expo, summed = G._oracle(at, cfg, dt)
        vel = second[k][1]
        if k >= dyn_first:
            needed = P.check_velocity_conditioned(vel[free], v_ref[free], expo[free], summed[free], dt)
            assert needed <= max(2, n // 100), f"scene {k}"
        else:
            P.check_velocity(vel[free], v_ref[free], expo[free], dt)
        if (~free).any():                                              # ... and the commands did move somebody
            assert not np.array_equal(first[k][0], _plain(z_spread)[1][k][0])


# ---- replay ---------------------------------------------------------------------------------------------------------------------

REPLAY_SIZES = (3, 65, 300)
REPLAY_DTS = (0.05, 0.04, 0.03)
REPLAY_T0 = (4.5, 4.5, 4.7)
K = 12
FEATURES = ("plain", "redraw", "tracks", "modes", "spawns")          # spawns: modes + spawn schedule + tracked vehicles


def _has(feat, what):
    return {"vehicles": feat in ("tracks", "modes", "spawns"), "tracks": feat in ("tracks", "spawns"),
            "modes": feat in ("modes", "spawns"), "spawns": feat == "spawns", "redraw": feat == "redraw"}[what]


@lru_cache(maxsize=None)
def _made(z3):
    made = [M._scene(n, 5100 + k, 2, z_spread=1.5 if z3 else 0.0, borders=2) for k, n in enumerate(REPLAY_SIZES)]
    scenes = [m[0] for m in made]
    plans = [scenarios.make_mode_plan(sc, 5150 + k, queue_len=1)[0] for k, sc in enumerate(scenes)]
    scheds = [scenarios.make_spawn_plan(sc, 5300 + k, dt=REPLAY_DTS[k], t0=REPLAY_T0[k], present=0.35, horizon=1.5)
              for k, sc in enumerate(scenes)]
    tracks = [scenarios.make_track_plan(sc, 5200 + k, K + 8, dt=REPLAY_DTS[k]) for k, sc in enumerate(scenes)]
    return scenes, plans, scheds, tracks


def _build(feat, z3=False, pick=None):
    scenes, plans, scheds, tracks = _made(z3)
    idx = list(range(len(REPLAY_SIZES))) if pick is None else list(pick)
    sub = lambda xs: [xs[k] for k in idx]
    b = SfmBatch([M._config(k) for k in idx], sub(REPLAY_DTS))
    try:
        b.upload(sub(scenes), device_vehicles=_has(feat, "vehicles"))
        assert b.planar == (not z3)
        if _has(feat, "redraw"):
            b.set_waypoint_streams([21 + k for k in idx], 30.0, 2.0)
        if _has(feat, "tracks"):
            b.set_vehicle_tracks(sub(tracks))
        if _has(feat, "modes"):
            b.set_modes(sub(plans), despawn_on_arrival=True, sim_time0=sub(REPLAY_T0), arrive_thresholds=2.0, scenes=sub(scenes))
        if _has(feat, "spawns"):
            b.set_spawns(sub(scheds))
    except Exception:
        b.close()
        raise
    return b


def _read(b, feat):
    out = [{"loc": loc, "vel": vel, "wp": wp, "draws": d, "ctr": [c for c, _ in veh], "ring": [r for _, r in veh]}
           for (loc, vel), (wp, d), veh in zip(b.state(), b.waypoints(), b.dynamic_obstacles())]
    if _has(feat, "modes"):
        clocks = b.clocks()
        for k, (m, t, c) in enumerate(b.modes()):
            out[k].update(mode=m, target=t, cursor=c, clock=clocks[k:k + 1])
    if _has(feat, "spawns"):
        for k, (born, when) in enumerate(b.spawns()):
            out[k].update(born=born, birth=when)
    if _has(feat, "tracks"):
        for k, p in enumerate(b.vehicle_tracks()[1]):
            out[k].update(present=p)
    return out


def _assert_batches(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        R._assert_scene(g, w, f"{what}: scene {k}")


@lru_cache(maxsize=None)
def _unsteered_run(feat, z3):
    """Batch A: its recorded run (frames, zframes, final state) and, from an identical batch stepped tick by tick, the readout
    after each tick."""
    a = _build(feat, z3)
    try:
        frames, _, zframes = a.run_recorded(K, redraw=_has(feat, "redraw"))
        final = a.state()
    finally:
        a.close()
    s = _build(feat, z3)
    try:
        reads = [_read(s, feat)]
        for _ in range(K):
            s.run(1, redraw=_has(feat, "redraw"))
            reads.append(_read(s, feat))
    finally:
        s.close()
    return frames, zframes, final, reads


@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
@pytest.mark.parametrize("feat", FEATURES)
def test_replaying_recorded_velocities_is_the_identity(feat, z3):
    """Batch B steers a seeded third of its rows (kind 1) with batch A's own recorded v' of every tick: after every tick everything
    readable of B equals A's, bit for bit -- rows that despawn, and rows that wait for their birth, among the steered ones."""
    frames, zframes, final, reads = _unsteered_run(feat, z3)
    rng = np.random.default_rng(314)
    kinds = [(rng.random(n) < 1.0 / 3.0).astype(np.uint8) for n in REPLAY_SIZES]
    assert sum(int(kd.sum()) for kd in kinds) > 50
    if _has(feat, "modes"):
        gone = [(r0["mode"] != M.GONE) & (r1["mode"] == M.GONE) for r0, r1 in zip(reads[0], reads[K])]
        assert sum(int((g & (kd == 1)).sum()) for g, kd in zip(gone, kinds)) > 0, "no steered row despawns during the run"
    if _has(feat, "spawns"):
        late = [~r0["born"] & r1["born"] for r0, r1 in zip(reads[0], reads[K])]
        never = [~r1["born"] for r1 in reads[K]]
        assert sum(int((g & (kd == 1)).sum()) for g, kd in zip(late, kinds)) > 0, "no steered row is born during the run"
        assert sum(int((g & (kd == 1)).sum()) for g, kd in zip(never, kinds)) > 0, "no steered row stays unborn"

    def command(t):                                                    # v' of tick t: the velocity of frame t + 1
        out = []
        for k, n in enumerate(REPLAY_SIZES):
            u = np.zeros((n, 3), np.float32)
            if t + 1 < K:
                u[:, :2] = frames[k][t + 1][:, 2:]
                if z3:
                    u[:, 2] = zframes[k][t + 1][:, 1]
            else:
                u[:] = final[k][1]
            out.append(u)
        return out

    b = _build(feat, z3)
    try:
        b.set_steering(kinds, command(0))
        _assert_batches(_read(b, feat), reads[0], f"{feat}: before the first tick")
        for t in range(K):
            if t:
                b.set_commands(command(t))
            b.run(1, redraw=_has(feat, "redraw"))
            _assert_batches(_read(b, feat), reads[t + 1], f"{feat}: after tick {t}")
        for k in range(len(REPLAY_SIZES)):                             # (the recorded run and the stepped one are one run)
            assert R._same_array(final[k][0], reads[K][k]["loc"]) and R._same_array(final[k][1], reads[K][k]["vel"])
    finally:
        b.close()


# ---- steering that steers nobody ----------------------------------------------------------------------------------------------

def _four_forms(feat, z3, steer):
    redraw = _has(feat, "redraw")
    out = []
    for form in range(4):
        b = _build(feat, z3)
        try:
            if steer:
                b.set_steering(0, [np.full(3, 7.0)] * len(REPLAY_SIZES))    # a command nobody follows
            if form == 0:
                b.run(8, redraw=redraw)
                extra = None
            elif form == 1:
                for _ in range(8):
                    b.tick(integrate=True, redraw=redraw)
                extra = None
            elif form == 2:
                extra = b.run_recorded(8, redraw=redraw)
            else:
                extra = b.run_recorded_forces(8, redraw=redraw)
            out.append((_read(b, feat), extra))
        finally:
            b.close()
    return out


def _same_nested(u, v):
    if isinstance(u, (list, tuple)):
        return len(u) == len(v) and all(_same_nested(a, c) for a, c in zip(u, v))
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(_same_nested(u[k], v[k]) for k in u)
    if u is None or v is None:
        return u is None and v is None
    return R._same_array(u, v)


@pytest.mark.parametrize("feat,z3", [("plain", False), ("plain", True), ("redraw", False), ("modes", True), ("spawns", False)])
def test_steering_with_every_kind_zero_is_a_no_op(feat, z3):
    """run(8), 8 x tick, run_recorded(8) and run_recorded_forces(8) with steering on and every kind 0: bitwise the batch without
    steering -- state, waypoints, modes, births, vehicles, frames and force records."""
    for form, ((got, gx), (want, wx)) in enumerate(zip(_four_forms(feat, z3, True), _four_forms(feat, z3, False))):
        _assert_batches(got, want, f"{feat}, form {form}")
        assert _same_nested(gx, wx), f"{feat}, form {form}: frames or forces"


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_a_scene_does_not_depend_on_the_rest_of_the_batch(z_spread):
    """In the mixed batch the scene without a steered row is bitwise what it is in the unsteered batch, and the entirely steered
    scene is bitwise what it is alone (B = 1) with its commands."""
    _, first, second, _ = _steered(z_spread)
    _, pfirst, psecond, _ = _plain(z_spread)
    for q in range(2):
        assert np.array_equal(first[UNSTEERED][q], pfirst[UNSTEERED][q]) and np.array_equal(second[UNSTEERED][q], psecond[UNSTEERED][q])
    forces, afirst, asecond, _ = _one_tick(z_spread, True, pick=[ALL_STEERED])
    for q in range(2):
        assert np.array_equal(first[ALL_STEERED][q], afirst[0][q]) and np.array_equal(second[ALL_STEERED][q], asecond[0][q])
    assert _same_nested(forces[0], _steered(z_spread)[0][ALL_STEERED])
    assert not np.array_equal(first[ALL_STEERED][1], pfirst[ALL_STEERED][1])


# ---- device pointers, lifetime, refusals ----------------------------------------------------------------------------------------

def _steer_plan(z3, seed=7):
    rng = np.random.default_rng(seed)
    kinds = [rng.integers(0, 3, n).astype(np.uint8) for n in REPLAY_SIZES]
    c0 = [np.float32(rng.uniform(-1.0, 1.0, (n, 3))) for n in REPLAY_SIZES]
    c1 = [np.float32(rng.uniform(-1.0, 1.0, (n, 3))) for n in REPLAY_SIZES]
    return kinds, c0, c1


@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
def test_device_tensors(z3):
    """Commands written through command_tensor() give bitwise the state set_commands gives; a kind flipped through the tensor
    takes effect in the next tick; state_tensor() is state_arrays(); the views are what sfm_batch_device_ptr reports."""
    import torch
    feat = "modes"
    kinds, c0, c1 = _steer_plan(z3)
    x = _build(feat, z3)
    try:
        x.set_steering(kinds, c0)
        x.run(1)
        x.set_commands(c1)
        x.run(3)
        want = _read(x, feat)
    finally:
        x.close()
    n = sum(REPLAY_SIZES)
    y = _build(feat, z3)
    try:
        y.set_stream(torch.cuda.current_stream().cuda_stream)
        y.set_steering(kinds, c0)
        cmd = y.command_tensor()
        ptr, nbytes = y.device_ptr(PTR_COMMANDS)
        assert cmd.shape == (n, 4) and cmd.dtype == torch.float32 and cmd.data_ptr() == ptr and nbytes == 16 * n
        kd, u = pack_steering(kinds, c0, y.scene_off)[0], np.concatenate(c0)
        assert np.array_equal(cmd.cpu().numpy(), np.column_stack([u, kd.astype(np.float32)]))
        y.run(1)
        cmd[:, :3] = torch.from_numpy(np.concatenate(c1)).to(cmd.device)
        y.run(3)
        _assert_batches(_read(y, feat), want, "command_tensor against set_commands")
        # the state views
        st = y.state_tensor()
        sptr, sbytes = y.device_ptr(PTR_STATE)
        assert st.shape == (n, 4) and st.data_ptr() == sptr and sbytes == 16 * n
        torch.cuda.synchronize()
        loc, vel = y.state_arrays()
        s = st.cpu().numpy().astype(np.float64)
        assert np.array_equal(s[:, :2], loc[:, :2]) and np.array_equal(s[:, 2:], vel[:, :2])
        zt = y.zstate_tensor()
        if z3:
            zptr, zbytes = y.device_ptr(PTR_ZSTATE)
            assert zt.shape == (n, 2) and zt.data_ptr() == zptr and zbytes == 8 * n
            z = zt.cpu().numpy().astype(np.float64)
            assert np.array_equal(z[:, 0], loc[:, 2]) and np.array_equal(z[:, 1], vel[:, 2])
        else:
            assert zt is None and y.device_ptr(PTR_ZSTATE) == (0, 0)
        # a kind flipped on the device: live velocity rows of the largest scene stop following their commands in the next tick
        s0 = int(y.scene_off[2])
        y.run(1)
        rows = np.flatnonzero((kinds[2] == 1) & (y.modes()[2][0] != M.GONE))[:5]     # (a row that despawned in the tick is parked)
        assert len(rows) == 5
        v = y.state()[2][1]
        assert np.array_equal(np.float32(v[rows][:, :2]), c1[2][rows][:, :2])
        cmd[torch.from_numpy(s0 + rows).to(cmd.device), 3] = 0.0
        y.run(1)
        v = y.state()[2][1]
        assert not (np.float32(v[rows][:, :2]) == c1[2][rows][:, :2]).all(axis=1).any()
        assert (y.steering()[2][0][rows] == 0).all()
    finally:
        y.close()


def test_lifetime():
    """set_params keeps steering, upload drops it, set_steering and set_commands keep the snapshot, and a restart leaves kinds and
    commands alone: the restarted scenes follow their commands again."""
    feat = "spawns"
    kinds, c0, c1 = _steer_plan(False, 11)
    scenes = _made(False)[0]
    b = _build(feat)
    try:
        with pytest.raises(SfmLibraryError, match="steering is off"):
            b.steering()
        b.snapshot()
        b.set_steering(kinds, c0)
        assert b.has_snapshot
        b.run(4)
        b.set_commands(c1)
        assert b.has_snapshot
        b.run(3)
        b.set_params([M._config(k + 1) for k in range(len(REPLAY_SIZES))], list(REPLAY_DTS))
        got = b.steering()
        for k in range(len(REPLAY_SIZES)):
            assert np.array_equal(got[k][0], kinds[k]) and np.array_equal(got[k][1][:, :2], c1[k][:, :2])
        b.set_params([M._config(k) for k in range(len(REPLAY_SIZES))], list(REPLAY_DTS))
        other = _read(b, feat)
        b.restart([1, 2])
        got = b.steering()
        for k in range(len(REPLAY_SIZES)):
            assert np.array_equal(got[k][0], kinds[k]) and np.array_equal(got[k][1][:, :2], c1[k][:, :2])
        b.run(4)
        after = _read(b, feat)
        # the reference: the same batch, steered with c1 from the start (what the snapshot held plus the commands of the moment)
        f = _build(feat)
        try:
            f.set_steering(kinds, c1)
            f.run(4)
            fresh = _read(f, feat)
        finally:
            f.close()
        for k in (1, 2):
            R._assert_scene(after[k], fresh[k], f"restarted scene {k}")
            born = after[k]["born"]
            rows = (kinds[k] == 1) & (after[k]["mode"] != M.GONE) & born
            assert rows.sum() > 3 and np.array_equal(np.float32(after[k]["vel"][rows][:, :2]), c1[k][rows][:, :2])
        assert after[0]["clock"][0] > other[0]["clock"][0]             # scene 0 went on
        b.upload(scenes, device_vehicles=True)
        with pytest.raises(SfmLibraryError, match="steering is off"):
            b.steering()
        with pytest.raises(SfmLibraryError, match="steering is off"):
            b.set_commands(c1)
        with pytest.raises(SfmLibraryError, match="steering is off"):
            b.command_tensor()
    finally:
        b.close()


def test_refusals_leave_the_batch_usable():
    """Every refusal returns an error whose message names the cause, launches nothing, and a following run(1) matches a batch that
    never saw the refused calls, bitwise."""
    feat = "modes"
    kinds, c0, c1 = _steer_plan(False, 13)
    n = sum(REPLAY_SIZES)
    a = SfmBatch([M._config(k) for k in range(len(REPLAY_SIZES))], list(REPLAY_DTS))
    L = a._lib
    err = lambda h: L.sfm_batch_last_error(h._b).decode()
    z = np.zeros(n, np.float32)
    try:
        kd = np.zeros(n, np.uint8)
        assert L.sfm_batch_set_steering(a._b, _lib.u8ptr(kd), _lib.fptr(z), _lib.fptr(z), None) == SFM_ERR_STATE
        assert "sfm_batch_upload_state has not been called" in err(a)
        assert L.sfm_batch_device_ptr(a._b, PTR_STATE, None) is None and "sfm_batch_upload_state has not been called" in err(a)
        with pytest.raises(SfmLibraryError, match="upload"):
            a.set_steering(kinds, c0)
    finally:
        a.close()
    want_off = _build(feat)
    want_on = _build(feat)
    try:
        want_off.run(1)
        want_on.set_steering(kinds, c0)
        want_on.run(1)
        off, on = _read(want_off, feat), _read(want_on, feat)
    finally:
        want_off.close()
        want_on.close()
    b = _build(feat)
    try:
        kd, ux, uy, uz = pack_steering(kinds, c0, b.scene_off)
        row = int(np.flatnonzero(kd != 0)[0])
        free = int(np.flatnonzero(kd == 0)[0])
        # while steering is off
        assert L.sfm_batch_set_commands(b._b, _lib.fptr(ux), _lib.fptr(uy), None) == SFM_ERR_STATE and "steering is off" in err(b)
        assert L.sfm_batch_download_steering(b._b, None, None, None, None) == SFM_ERR_STATE and "steering is off" in err(b)
        assert L.sfm_batch_device_ptr(b._b, PTR_COMMANDS, None) is None and "steering is off" in err(b)
        assert L.sfm_batch_device_ptr(b._b, 3, None) is None and "which" in err(b)
        bad = kd.copy()
        bad[row] = 3
        assert L.sfm_batch_set_steering(b._b, _lib.u8ptr(bad), _lib.fptr(ux), _lib.fptr(uy), _lib.fptr(uz)) == SFM_ERR_INVALID
        assert f"row {row}: kind must be 0" in err(b)
        assert L.sfm_batch_set_steering(b._b, _lib.u8ptr(kd), None, _lib.fptr(uy), None) == SFM_ERR_INVALID and "NULL" in err(b)
        for col in range(3):
            for val in (np.nan, np.inf):
                cols = [ux.copy(), uy.copy(), uz.copy()]
                cols[col][row] = val
                assert L.sfm_batch_set_steering(b._b, _lib.u8ptr(kd), *(_lib.fptr(c) for c in cols)) == SFM_ERR_INVALID
                assert f"row {row}: the command of a steered row is not finite" in err(b)
        with pytest.raises(ValueError, match="finite"):
            b.set_steering(kinds, [np.full((nn, 3), np.nan, np.float32) for nn in REPLAY_SIZES])
        with pytest.raises(SfmLibraryError, match="steering is off"):
            b.steering()                                               # none of them switched it on
        c = _build(feat)
        try:
            c.run(1)
            _assert_batches(_read(c, feat), off, "(sanity) two unsteered batches")
        finally:
            c.close()
        b.run(1)
        _assert_batches(_read(b, feat), off, "after the refused set_steering calls")
    finally:
        b.close()
    b = _build(feat)
    try:
        b.set_steering(kinds, c0)
        kd, ux, uy, uz = pack_steering(kinds, c0, b.scene_off)
        row, free = int(np.flatnonzero(kd != 0)[0]), int(np.flatnonzero(kd == 0)[0])
        nan = ux.copy()
        nan[row] = np.nan
        assert L.sfm_batch_set_commands(b._b, _lib.fptr(nan), _lib.fptr(uy), _lib.fptr(uz)) == SFM_ERR_INVALID
        assert f"row {row}: the command of a steered row is not finite" in err(b)
        assert L.sfm_batch_set_commands(b._b, _lib.fptr(ux), None, None) == SFM_ERR_INVALID and "NULL" in err(b)
        bad = kd.copy()
        bad[free] = 200
        assert L.sfm_batch_set_steering(b._b, _lib.u8ptr(bad), _lib.fptr(ux), _lib.fptr(uy), _lib.fptr(uz)) == SFM_ERR_INVALID
        got = b.steering()                                             # kinds and commands as they were
        for k in range(len(REPLAY_SIZES)):
            assert np.array_equal(got[k][0], kinds[k]) and np.array_equal(got[k][1], c0[k])
        ok = ux.copy()
        ok[free] = np.nan                                              # a row that is not steered may hold anything
        assert L.sfm_batch_set_commands(b._b, _lib.fptr(ok), _lib.fptr(uy), _lib.fptr(uz)) == 0
        b.run(1)
        _assert_batches(_read(b, feat), on, "after the refused set_commands calls")
    finally:
        b.close()
