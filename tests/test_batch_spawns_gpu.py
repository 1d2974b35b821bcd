"""GPU tests of the batch's spawn schedule (sfm_batch_set_spawn_schedule, sfm_batch_download_spawns; SfmBatch.set_spawns / spawns):
every tick of every scene against the reference's host loop with births, same-tick visibility of a newborn, a schedule that
changes nothing, restart from a downloaded state, scene independence, the run forms, set_params, refused input and a batch at
size.  Helpers (scenes, configs, the host loop's force / mode half) are those of test_batch_modes_gpu.py.
Run on the MI355X box with  python -m pytest tests/test_batch_spawns_gpu.py -m gpu."""
import numpy as np
import pytest

import _parity as P
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import SfmBatch, pack_spawns
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.ped_mode_manager import PedMode
from carla_social_force_model_amd.spawner import MODE_UNBORN, birth_ticks, births
from oracle import sfm_oracle as O
from test_batch_modes_gpu import GONE, _advance, _assert_same, _batch, _config, _Host, _park, _scene

pytestmark = pytest.mark.gpu

SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3


def _parked(i):
    """park_position(i) as the device computes it: one fused multiply-add, FAR_AWAY + FAR_STEP * (i + 1) rounded once (the
    products are exact in float64).  It differs by an ulp from the two-rounding form for 77 of the indices below 1024, the first
    being 283."""
    return np.array([np.float32(float(np.float32(3.0e15)) + float(np.float32(1.0e12)) * (i + 1)), np.float32(-3.0e15)], dtype=np.float64)


def _f32(a):
    return np.float32(a).astype(np.float64)


def _spawn_batch(scenes, plans, scheds, cfgs, dts, despawn=True, t0=0.0, thr=2.0, planar=None):
    b = _batch(scenes, plans, cfgs, dts, despawn, t0, thr, planar)
    b.set_spawns(scheds)
    return b


def _all(b):
    """State, waypoints, modes, targets, cursors, born flags and birth clocks of every scene, and the clocks (NaN as bits)."""
    rows = [(loc, vel, wp, m, t, c, born, when.view(np.uint32))
            for (loc, vel), (wp, _), (m, t, c), (born, when) in zip(b.state(), b.waypoints(), b.modes(), b.spawns())]
    return rows, b.clocks()


class _SpawnHost(_Host):
    """test_batch_modes_gpu._Host with births: an unborn row is not alive (a ghost without a mode tick, like a despawned one) until
    the host twin of the birth rule -- on the float32 clock the device reports -- lets it in at its spawn state."""

    def __init__(self, sc, plan, ms, cfg, dt, thr, despawn, sched, clock0):
        super().__init__(sc, plan, ms, cfg, dt, thr, despawn)
        self.st, self.chain = sched["spawn_time"], sched["chain"]
        self.born = np.zeros(self.n, bool)          # (the rows the device keeps live at set time are born in the twin's first tick)
        self.when = np.full(self.n, np.nan, dtype=np.float32)
        self.gone = np.zeros(self.n, bool)
        self.loc0, self.vel0 = _f32(sc["loc"]), _f32(sc["vel"])
        self.alive[:] = self.born

    def tick(self, loc, vel, wp2, vehicles, now, ev, t):
        new = births(self.born, self.st, self.chain, now) & ~self.born
        due = (self.st <= np.float32(now)) & ~self.born
        ev["born_later"] += int(new.sum()) if t else 0
        ev["chain_delayed"] += int((due & ~new).sum() > 0)
        loc, vel = loc.copy(), vel.copy()
        z = loc[new, 2]
        loc[new], vel[new] = self.loc0[new], self.vel0[new]
        if not self.z3:
            loc[new, 2] = z
        self.born |= new
        self.when[new] = np.float32(now)
        self.alive[new] = True
        self.new = new
        out = super().tick(loc, vel, wp2, vehicles, float(now), ev)
        ev["newborn_checking"] += sum(self.ms[i].current_mode == PedMode.CHECKING_TRAFFIC for i in np.nonzero(new)[0])
        ev["born_then_despawned"] += int((~self.alive & self.born & ~self.gone & (self.when > np.float32(self.clock0))).sum())
        self.gone = ~self.alive & self.born
        return out


def test_every_tick_matches_the_host_loop():
    """Scenes of 0, 1, 2, 65, 200 and 1000 rows (every slice shape), their own step lengths, with and without despawn, one batch
    planar and one 3-D (smaller): who is born (exactly: both sides compare the same float32 numbers), modes with 254 / 255, cursors,
    targets, waypoints, ghosts at park_position, birth clocks and v' of every scene against the reference's host loop on the
    device's state, under the tolerances of test_batch_modes_gpu.py.  The rows are make_scenario's (spread out), the schedules
    make_spawn_plan's; births on the host side come from the NumPy twin of the birth rule, which test_batch_spawns_host.py pins to
    the reference's PedSpawner (the test below drives a scene with the mirror spawners themselves).  Ghosts are held to the
    device's fused park_position (_parked).  Seeds tried: 2900 (planar) and 2950 (3-D) only."""
    for z_spread, sizes, ticks, seed in ((0.0, (0, 1, 2, 65, 200, 1000, 40), 120, 2900), (1.5, (2, 65, 130), 40, 2950)):
        B = len(sizes)
        dts = [(0.05, 0.04, 0.05, 0.03, 0.05, 0.04, 0.05)[k] for k in range(B)]
        despawn = [k % 2 == 0 for k in range(B)]
        t0 = [(4.0, 3.0, 4.5, 3.5, 4.0, 3.0, 2.5)[k] for k in range(B)]
        thr = 2.0
        made = [_scene(n, seed + k, 4 if n else 2, z_spread) for k, n in enumerate(sizes)]
        scenes, plans = [m[0] for m in made], [m[1] for m in made]
        # the last planar scene: everybody unborn for the first ticks
        scheds = [scenarios.make_spawn_plan(sc, seed + 50 + k, dt=dts[k], t0=t0[k], present=0.0 if k == 6 else 0.35, horizon=2.0)
                  for k, sc in enumerate(scenes)]
        cfgs = [_config(k) for k in range(B)]
        b = _spawn_batch(scenes, plans, scheds, cfgs, dts, despawn, t0, thr, planar=z_spread == 0.0)
        hosts = []
        for k in range(B):
            h = _SpawnHost(scenes[k], plans[k], made[k][2], cfgs[k], dts[k], thr, despawn[k], scheds[k], np.float32(t0[k]))
            h.z3, h.clock0 = z_spread != 0.0, t0[k]
            hosts.append(h)
        ev = dict(idle_wake=0, waiting=0, checking=0, crossing=0, road_to_sidewalk=0, despawn=0, popped=0, born_later=0,
                  chain_delayed=0, newborn_checking=0, born_then_despawned=0, all_unborn=0)
        clock = np.float32(t0)
        try:
            for t in range(ticks):
                assert np.array_equal(b.clocks(), clock), f"clocks before tick {t}"
                state, wps, veh = b.state(), b.waypoints(), b.dynamic_obstacles()
                expect = {}
                for k, h in enumerate(hosts):
                    if h.n == 0 or (h.n > 500 and t >= 8):
                        continue
                    loc, vel = state[k]
                    ev["all_unborn"] += t > 0 and h.n > 1 and not h.born.any()
                    expect[k] = h.tick(loc, vel, wps[k][0].astype(np.float64), veh[k], clock[k], ev, t)
                b.run(1)
                clock = (clock + np.float32(dts)).astype(np.float32)
                after, wps2, modes, sp = b.state(), b.waypoints(), b.modes(), b.spawns()
                for k, (v_new, wp, unsure, diag) in expect.items():
                    h = hosts[k]
                    born, when = sp[k]
                    assert np.array_equal(born, h.born), f"scene {k} tick {t}: births differ at {np.nonzero(born != h.born)[0][:5]}"
                    assert np.array_equal(when.view(np.uint32), h.when.view(np.uint32)), f"scene {k} tick {t}: birth clocks"
                    m, tg, cur = (a.copy() for a in modes[k])
                    un = ~h.born
                    assert (m[un] == MODE_UNBORN).all() and not tg[un].any() and not cur[un].any(), f"scene {k} tick {t}: unborn modes"
                    ghost = un | (m == GONE)                      # (what the device itself calls a ghost)
                    for i in np.nonzero(ghost)[0]:
                        assert np.array_equal(after[k][0][i, :2], _parked(i)) and not after[k][1][i].any(), f"scene {k} tick {t}: ghost {i}"
                    assert np.array_equal(wps2[k][0][un], np.float32(scenes[k]["waypoint"][un, :2])), f"scene {k} tick {t}: unborn waypoints"
                    # the parent check sees an unborn row as it sees a despawned one: not alive, mode 255, parked -- where its own
                    # _park (two roundings) is an ulp off the device's fused form, the row was checked above and is handed over there
                    m[un] = GONE
                    loc_after = after[k][0].copy()
                    for i in np.nonzero(ghost)[0]:
                        loc_after[i, :2] = _park(i)
                    h.check(k, t, loc_after, after[k][1], wps2[k][0].astype(np.float64), m, tg, cur, v_new, wp, unsure, diag)
                for sc, dt in zip(scenes, dts):
                    _advance(sc, dt)
            print(f"\nspawn host loop z_spread={z_spread}: {ev}")
            assert ev["born_later"] > 20 and ev["chain_delayed"] > 5, ev
            if z_spread == 0.0:
                assert ev["newborn_checking"] > 0 and ev["born_then_despawned"] > 0 and ev["all_unborn"] > 0, ev
                assert ev["popped"] > 50 and ev["despawn"] > 3, ev
        finally:
            b.close()


def test_mirror_spawners_drive_the_host_loop():
    """A scene expanded from PedSpawner mirrors (scene_from_spawners: six spawners of four pedestrians at spread-out locations,
    intervals above the step length, one below it and one that starts behind the clock), the host loop's births decided by
    the mirrors themselves the way PedSpawnManager.tick does -- ready_to_spawn(clock the device reports), one release per spawner
    per tick -- and everything else as in the test above.  Spawn times sit off the clock's grid, so the float64 comparison of
    the mirror and the float32 one of the device see the same order.  Seeds tried: 3100 only."""
    from carla_social_force_model_amd.spawner import PedSpawner, scene_from_spawners
    seed, dt, t0, thr, ticks = 3100, 0.05, 1.0, 2.0, 90
    base, _, _ = _scene(24, seed, 2)
    rng = np.random.default_rng(seed)
    spawners = []
    for s_ in range(6):
        x = base["loc"][4 * s_].copy()
        wps = np.cumsum(np.concatenate([[x], np.c_[rng.uniform(-4.0, 4.0, (3, 2)), np.zeros(3)]]), axis=0)[1:]
        start = t0 - 0.12 if s_ == 0 else t0 + 0.013 + float(rng.uniform(0.0, 1.0))
        interval = (0.4, 0.61, 0.02, 0.83, 0.47, 1.1)[s_]
        spawners.append(PedSpawner(np.float32(x).astype(np.float64), np.float32(wps).astype(np.float64), [False, bool(s_ % 2), True],
                                   1.0 + 0.1 * s_, None, 4, start, interval, 1.5, -1.0 if s_ % 3 == 0 else 1.0))
    rows, plan, sched, managers = scene_from_spawners(spawners, radius=0.3)
    sc = dict(base)
    sc.update(rows)
    cfg = _config(0)
    b = _spawn_batch([sc], [plan], [sched], [cfg], [dt], True, t0, thr)
    h = _SpawnHost(sc, plan, managers, cfg, dt, thr, True, sched, np.float32(t0))
    h.z3, h.clock0 = False, t0
    ev = dict(idle_wake=0, waiting=0, checking=0, crossing=0, road_to_sidewalk=0, despawn=0, popped=0, born_later=0,
              chain_delayed=0, newborn_checking=0, born_then_despawned=0)
    clock = np.float32(t0)
    released = np.zeros(24, bool)
    try:
        for t in range(ticks):
            (loc, vel), (wp, _), veh = b.state()[0], b.waypoints()[0], b.dynamic_obstacles()[0]
            assert b.clocks()[0] == clock
            for s_, sp in enumerate(spawners):                      # PedSpawnManager.tick on the mirrors
                if sp.quantity > 0 and sp.ready_to_spawn(float(clock)):
                    released[4 * s_ + 4 - sp.quantity] = True
                    sp.quantity -= 1
            v_new, wp1, unsure, diag = h.tick(loc, vel, wp.astype(np.float64), veh, clock, ev, t)
            assert np.array_equal(h.born, released), f"tick {t}: the twin and the mirrors disagree"
            b.run(1)
            clock = np.float32(clock + np.float32(dt))
            (loc1, vel1), (wp2, _), (m, tg, cur), (born, when) = b.state()[0], b.waypoints()[0], b.modes()[0], b.spawns()[0]
            assert np.array_equal(born, released), f"tick {t}: births differ at {np.nonzero(born != released)[0]}"
            assert np.array_equal(when.view(np.uint32), h.when.view(np.uint32)), f"tick {t}: birth clocks"
            m, un = m.copy(), ~released
            assert (m[un] == MODE_UNBORN).all()
            m[un] = GONE
            h.check(0, t, loc1, vel1, wp2.astype(np.float64), m, tg, cur, v_new, wp1, unsure, diag)
            _advance(sc, dt)
        print(f"\nmirror spawners: {ev}")
        assert released.all() and ev["born_later"] >= 18 and ev["chain_delayed"] >= 2 and ev["popped"] > 10, ev
    finally:
        b.close()


def test_a_newborn_is_part_of_its_birth_tick():
    """Two rows 0.5 m apart, the second born in tick T = 3: the first row's pedestrian force is exactly 0 in tick T - 1 and the
    oracle's two-body force (1e-5) in tick T; the newborn's own record is zeros in T - 1 and the oracle's in T."""
    cfg = default_sfm_config(("acceleration_force", "pedestrian_force"))
    dt, T = 0.05, 3
    sc = vars(scenarios.make_scenario(2, 11))
    sc["loc"] = np.array([[1.0, 2.0, 0.0], [1.5, 2.0, 0.0]])
    sc["vel"] = np.array([[0.0, 0.0, 0.0], [0.3, 0.4, 0.0]])          # row 0 at rest with waypoint = position and target 0: it stays
    sc["waypoint"] = np.array([[1.0, 2.0, 0.0], [9.0, 2.0, 0.0]])
    sc["target_speed"] = np.array([0.0, 1.2])
    sc["radius"] = np.array([0.3, 0.3])
    plan, _ = scenarios.make_mode_plan(sc, 1, queue_len=0, idle_every=0)
    sc["waypoint"] = np.array([[1.0, 2.0, 0.0], [9.0, 2.0, 0.0]])      # (make_mode_plan rewrote them)
    sched = {"spawn_time": np.float32([-np.inf, T * dt - 0.01]), "chain": [0, 0]}
    b = SfmBatch([cfg], [dt])
    try:
        b.upload([sc])
        b.set_modes([plan], despawn_on_arrival=False, arrive_thresholds=0.0)
        b.set_spawns([sched])
        now = np.float32(0.0)
        for t in range(T + 1):
            before, now = now, np.float32(now + np.float32(dt))
            (loc, vel), = b.state()
            (rec,) = b.tick_forces(integrate=False)
            (born, when), = b.spawns()
            if t < T:
                assert not born[1] and np.isnan(when[1])
                assert not rec["pedestrian_force"].any() and not rec["total"][1].any() and not rec["acceleration_force"][1].any(), t
                assert np.array_equal(loc[1, :2], _parked(1))
                continue
            assert born[1] and when[1] == before and b.clocks()[0] == now
            prm = O.OracleParams.from_config(cfg)
            geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"], sc["dynamic_obstacles"],
                              sc["dynamic_vel"])
            with np.errstate(all="ignore"):
                ref, total, _ = O.tick_forces(_f32(sc["loc"]), _f32(sc["vel"]), sc["waypoint"], sc["target_speed"], sc["radius"],
                                              np.zeros(2, bool), geom, prm, theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL)
            scale = np.abs(ref["pedestrian_force"]).max()
            assert scale > 1e-3
            for name in ("pedestrian_force", "acceleration_force"):
                assert np.allclose(rec[name], ref[name][:, :2], rtol=1e-5, atol=1e-5 * scale), (name, rec[name], ref[name])
            assert np.allclose(rec["total"], total[:, :2], rtol=1e-5, atol=1e-5 * scale)
    finally:
        b.close()


def _two(sizes=(64, 17, 0, 130), seed=300, z=0.0):
    made = [_scene(n, seed + k, 3 if n else 1, z) for k, n in enumerate(sizes)]
    scenes, plans = [m[0] for m in made], [m[1] for m in made]
    cfgs = [_config(k) for k in range(len(sizes))]
    dts = [(0.05, 0.04, 0.02, 0.05)[k % 4] for k in range(len(sizes))]
    return scenes, plans, cfgs, dts


def test_a_schedule_of_live_rows_changes_nothing():
    """Every row due at the start (-inf, or a time <= the clock, chain 0): state, waypoints, modes, clocks and force records over a
    run are bitwise those of the same batch without set_spawns."""
    scenes, plans, cfgs, dts = _two()
    scheds = [{"spawn_time": np.where(np.arange(len(sc["loc"])) % 2, -np.inf, 3.0), "chain": None} for sc in scenes]
    scheds[1] = None
    plain = _batch(scenes, plans, cfgs, dts, t0=4.0)
    sched = _spawn_batch(scenes, plans, scheds, cfgs, dts, t0=4.0)
    try:
        for born, when in sched.spawns():
            assert born.all() and (when == np.float32(4.0)).all()
        for b in (plain, sched):
            b.run(7)
        fa, ia, _, ra = plain.run_recorded_forces(12, stride=3)
        fb, ib, _, rb = sched.run_recorded_forces(12, stride=3)
        for s in range(len(scenes)):
            assert np.array_equal(fa[s].view(np.uint32), fb[s].view(np.uint32)), f"scene {s}: frames"
            for name in ra[s]:
                assert np.array_equal(ra[s][name].view(np.uint32), rb[s][name].view(np.uint32)), f"scene {s}: {name}"
        for b in (plain, sched):
            b.tick()
            b.run(20)
        assert np.array_equal(sched.clocks(), plain.clocks())
        a = _all(sched)
        rows = [(loc, vel, wp, m, t, cu) for (loc, vel), (wp, _), (m, t, cu) in zip(plain.state(), plain.waypoints(), plain.modes())]
        for s, (x, y) in enumerate(zip(a[0], rows)):
            for q, (u, v) in enumerate(zip(x[:6], y)):
                assert np.array_equal(u, v), f"scene {s} field {q}"
        sched.set_spawns(None)                                  # nobody unborn: the schedule may go
        with pytest.raises(_lib.SfmLibraryError, match="sfm_batch_set_spawn_schedule"):
            sched.spawns()
    finally:
        plain.close()
        sched.close()


@pytest.mark.parametrize("n", [40, 100, 300], ids=["4-slices", "2-slices", "1-slice"])
def test_restart_from_the_tick_before_a_birth(n):
    """Run to just before the last row's birth tick, download everything, build a second batch without a schedule whose upload has
    the newborn at its spawn state and the others where they are (modes, targets, cursors via shortened queues, clock via
    sim_time0): from that tick on both agree bitwise.  Nobody is a ghost at that point (no despawn; every other row born)."""
    sc, plan, _ = _scene(n, 700 + n, 0)                                # (no vehicles: a re-upload would regenerate their rings on the host)
    cfg, dt, t0 = _config(1), 0.05, 1.0
    K = 9
    st = np.full(n, -np.inf)
    st[n // 2:] = t0 + dt * np.arange(n - n // 2) * 0.01               # all due by tick 1 ...
    st[-1] = t0 + (K + 0.5) * dt                                       # ... but the last one: born in tick K + 1
    sched = {"spawn_time": st, "chain": np.zeros(n)}
    a = _spawn_batch([sc], [plan], [sched], [cfg], [dt], False, t0)
    c = None
    try:
        a.run(K + 1)
        (born, _), = a.spawns()
        assert born[:-1].all() and not born[-1]
        (loc, vel), (wp, _), (m, tg, cur), clk = a.state()[0], a.waypoints()[0], a.modes()[0], a.clocks()
        sc2 = dict(sc)
        sc2["loc"], sc2["vel"] = loc.copy(), vel.copy()
        sc2["loc"][-1], sc2["vel"][-1] = _f32(sc["loc"][-1]), _f32(sc["vel"][-1])
        sc2["waypoint"] = np.concatenate([wp.astype(np.float64), sc["waypoint"][:, 2:]], axis=1)
        plan2 = dict(plan)
        plan2["mode"], plan2["target_speed"] = m.astype(np.int64), tg.astype(np.float64)
        plan2["mode"][-1], plan2["target_speed"][-1] = plan["mode"][-1], plan["target_speed"][-1]
        plan2["queues"] = [list(q)[cur[i]:] for i, q in enumerate(plan["queues"])]
        c = _batch([sc2], [plan2], [cfg], [dt], False, float(clk[0]))
        assert c.clocks()[0] == clk[0]
        for step in range(12):
            a.run(1)
            c.run(1)
            (la, va), (lc, vc) = a.state()[0], c.state()[0]
            assert np.array_equal(la, lc) and np.array_equal(va, vc), f"tick {step} after the restart: state"
            (ma, ta, ca), (mc, tc, cc) = a.modes()[0], c.modes()[0]
            assert np.array_equal(ma, mc) and np.array_equal(ta, tc) and np.array_equal(ca, cc + cur), f"tick {step}: modes"
            assert np.array_equal(a.waypoints()[0][0], c.waypoints()[0][0])
        assert a.spawns()[0][0].all() and a.spawns()[0][1][-1] == clk[0]
    finally:
        a.close()
        if c is not None:
            c.close()


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_scene_is_independent_of_the_batch(z_spread):
    """A scene with a spawn schedule, alone and at positions 0, 2 and 5 of a batch of 6 mixed scenes, over 80 ticks: everything
    bitwise identical, births included."""
    target = _scene(65, 77, 4, z_spread)
    tcfg, tdt = _config(3), 0.04
    tsched = scenarios.make_spawn_plan(target[0], 5, dt=tdt, t0=1.0, horizon=2.0)
    others = [_scene(n, 1100 + k, m, z_spread) for k, (n, m) in enumerate(((30, 2), (0, 1), (250, 3)))]
    made = [target, others[0], target, others[1], others[2], target]
    cfgs = [tcfg, _config(0), tcfg, _config(1), _config(2), tcfg]
    dts = [tdt, 0.05, tdt, 0.05, 0.03, tdt]
    t0 = [1.0, 0.0, 1.0, 2.0, 0.5, 1.0]
    scheds = [tsched, scenarios.make_spawn_plan(others[0][0], 6), tsched, None, scenarios.make_spawn_plan(others[2][0], 7, t0=0.5),
              tsched]
    planar = z_spread == 0.0
    alone = _spawn_batch([target[0]], [target[1]], [tsched], [tcfg], [tdt], True, 1.0, planar=planar)
    mixed = _spawn_batch([m[0] for m in made], [m[1] for m in made], scheds, cfgs, dts, True, t0, planar=planar)
    try:
        for b in (alone, mixed):
            b.run(30)
            b.tick(integrate=True)
            b.tick()
            b.run(48)
        (a, ca), (m, cm) = _all(alone), _all(mixed)
        for pos in (0, 2, 5):
            _assert_same((a, ca), (m[pos:pos + 1], cm[pos:pos + 1]), f"alone vs position {pos}")
        born, when = alone.spawns()[0]
        assert born.sum() > (~np.isinf(tsched["spawn_time"])).sum() // 2 and (when[born] > 1.0).any()
    finally:
        alone.close()
        mixed.close()


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_run_forms_agree(z_spread):
    """run(K) == K x run(1) == K x tick(integrate=True) == the end of run_recorded == of run_recorded_forces == K x
    tick_forces(integrate=True), bit for bit, births included; frames == step-wise downloads (a frame holds the state before its
    tick: an unborn row's ghost, in its birth tick too)."""
    scenes, plans, cfgs, dts = _two(z=z_spread)
    scheds = [scenarios.make_spawn_plan(sc, 20 + k, dt=dts[k], t0=4.0, horizon=1.5) for k, sc in enumerate(scenes)]
    K = 30
    bs = [_spawn_batch(scenes, plans, scheds, cfgs, dts, t0=4.0, planar=z_spread == 0.0) for _ in range(6)]
    try:
        bs[0].run(K)
        want, wantz = [[] for _ in scenes], [[] for _ in scenes]
        for _ in range(K):
            for s, (loc, vel) in enumerate(bs[1].state()):
                want[s].append(np.float32(np.concatenate([loc[:, :2], vel[:, :2]], axis=1)))
                wantz[s].append(np.float32(np.stack([loc[:, 2], vel[:, 2]], axis=1)))
            bs[1].run(1)
            bs[2].tick(integrate=True)
            bs[5].tick_forces(integrate=True)
        frames, idx, zframes = bs[3].run_recorded(K)
        frames2, _, zframes2, _ = bs[4].run_recorded_forces(K, forces=["total"])
        ref = _all(bs[0])
        for k in range(1, 6):
            _assert_same(ref, _all(bs[k]), f"run({K}) vs form {k}")
        for s, sc in enumerate(scenes):
            w = np.stack(want[s]).reshape(K, len(sc["loc"]), 4) if len(sc["loc"]) else frames[s]
            assert np.array_equal(frames[s].view(np.uint32), w.view(np.uint32)), f"scene {s}: frames"
            assert np.array_equal(frames2[s].view(np.uint32), w.view(np.uint32)), f"scene {s}: frames beside forces"
            if z_spread and len(sc["loc"]):
                wz = np.stack(wantz[s]).reshape(K, len(sc["loc"]), 2)
                for zf in (zframes, zframes2):
                    assert np.array_equal(zf[s].view(np.uint32), wz.view(np.uint32)), f"scene {s}: z frames"
        assert sum(int((when > np.float32(4.0)).sum()) for _, when in bs[0].spawns()) > 20
    finally:
        for b in bs:
            b.close()


def test_set_params_keeps_the_schedule_and_moves_later_births():
    """A new step length mid-run: the schedule stays, and the births after it fall where the host twin says for the new clock."""
    sc, plan, _ = _scene(64, 55, 2)
    cfg = _config(0)
    sched = scenarios.make_spawn_plan(sc, 9, dt=0.05, t0=0.0, horizon=3.0)
    b = _spawn_batch([sc], [plan], [sched], [cfg], [0.05])
    try:
        born, when = np.zeros(64, bool), np.full(64, np.nan, dtype=np.float32)
        now = np.float32(0.0)
        for dt, K in ((0.05, 10), (0.02, 25), (0.1, 20)):
            b.set_params([cfg], [dt])
            b.run(K)
            for _ in range(K):
                new = births(born, sched["spawn_time"], sched["chain"], now) & ~born
                when[new] = now
                born |= new
                now = np.float32(now + np.float32(dt))
            (dborn, dwhen), = b.spawns()
            assert b.clocks()[0] == now
            assert np.array_equal(dborn, born) and np.array_equal(dwhen.view(np.uint32), when.view(np.uint32)), f"after dt={dt}"
        assert born.sum() > 40
    finally:
        b.close()


def test_refusals_leave_the_batch_unchanged():
    """No modes, NULL chain, a bad chain value, chain = 1 on a scene's first row, NaN, wrong lengths (the packer), a second schedule,
    switching off while a row is unborn, redraw=True: refused with a message, the batch bitwise unchanged and running on as a fresh
    one.  upload, set_modes and set_modes(None) drop the schedule."""
    L = _lib.load()
    scenes, plans, cfgs, dts = _two((20, 10), 81)
    scheds = [scenarios.make_spawn_plan(sc, 3 + k, dt=dts[k]) for k, sc in enumerate(scenes)]
    t, c = pack_spawns(scheds, np.array([0, 20, 30]))
    p = lambda a: None if a is None else a.ctypes.data
    nomodes = SfmBatch(cfgs, dts)
    b = _batch(scenes, plans, cfgs, dts)
    fresh = _spawn_batch(scenes, plans, scheds, cfgs, dts)
    try:
        nomodes.upload(scenes)
        assert L.sfm_batch_set_spawn_schedule(nomodes._b, p(t), p(c)) == SFM_ERR_STATE
        assert "sfm_batch_set_mode_fsm" in L.sfm_batch_last_error(nomodes._b).decode()
        assert L.sfm_batch_download_spawns(nomodes._b, None, None) == SFM_ERR_STATE
        before = [(loc, vel, wp, m, tg, cu) for (loc, vel), (wp, _), (m, tg, cu) in zip(b.state(), b.waypoints(), b.modes())]
        nan, two, first = t.copy(), c.copy(), c.copy()
        nan[5] = np.nan
        two[7] = 2
        first[20] = 1
        for args, msg in (((t, None), "chain is NULL"), ((nan, c), "NaN"), ((t, two), "0 or 1"), ((t, first), "first row")):
            assert L.sfm_batch_set_spawn_schedule(b._b, p(args[0]), p(args[1])) == SFM_ERR_INVALID, msg
            assert msg in L.sfm_batch_last_error(b._b).decode(), msg
        with pytest.raises(ValueError, match="rows, expected"):
            b.set_spawns([{"spawn_time": np.zeros(19)}, None])
        with pytest.raises(ValueError, match="2 spawn schedules|1 spawn schedules"):
            b.set_spawns([None])
        after = [(loc, vel, wp, m, tg, cu) for (loc, vel), (wp, _), (m, tg, cu) in zip(b.state(), b.waypoints(), b.modes())]
        for x, y in zip(before, after):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)
        with pytest.raises(_lib.SfmLibraryError, match="sfm_batch_set_spawn_schedule"):
            b.spawns()                                               # no schedule came into being
        b.set_spawns(scheds)
        b.run(4)
        fresh.run(4)
        snap = _all(b)
        with pytest.raises(_lib.SfmLibraryError, match="already been set"):
            b.set_spawns(scheds)
        with pytest.raises(_lib.SfmLibraryError, match="unborn"):
            b.set_spawns(None)
        with pytest.raises(_lib.SfmLibraryError, match="SFM_TICK_INTEGRATE"):
            b.run(2, redraw=True)
        _assert_same(snap, _all(b), "after the refused calls")
        b.run(6)
        fresh.run(6)
        _assert_same(_all(b), _all(fresh), "refused calls vs a fresh batch")
        b.set_modes(plans, scenes=scenes)                            # the modes anew: the schedule is gone
        with pytest.raises(_lib.SfmLibraryError, match="sfm_batch_set_spawn_schedule"):
            b.spawns()
        assert (b.modes()[0][0] != MODE_UNBORN).all()
        b.upload(scenes, device_vehicles=True)
        b.set_modes(plans, scenes=scenes)
        b.set_spawns(scheds)                                         # upload + set_modes: a schedule may be set again
        b.run(2)
        b.set_modes(None)
        assert L.sfm_batch_download_spawns(b._b, None, None) == SFM_ERR_STATE
    finally:
        for x in (b, fresh, nomodes):
            x.close()


def test_at_size():
    """1024 scenes x 64 rows, all five forces, 4 moving vehicles and modes each, a quarter of the rows arriving over 120 ticks:
    births at the host twin's ticks (clock values bitwise), every scene finite and bounded, unborn and despawned rows parked."""
    B, T = 1024, 120
    made = [_scene(64, 6000 + k, 4, borders=2) for k in range(B)]
    scenes, plans = [m[0] for m in made], [m[1] for m in made]
    cfgs = [_config(2 * (k % 2)) for k in range(B)]
    dts = [(0.05, 0.04, 0.02, 0.03)[k % 4] for k in range(B)]
    t0 = [float(k % 5) for k in range(B)]
    scheds = [scenarios.make_spawn_plan(sc, 40 + k, dt=dts[k], t0=t0[k], present=0.75, horizon=T * dts[k]) for k, sc in enumerate(scenes)]
    b = _spawn_batch(scenes, plans, scheds, cfgs, dts, True, t0)
    try:
        b.run(T)
        state, modes, sp = b.state(), b.modes(), b.spawns()
        late = 0
        for k in range(B):
            (loc, vel), (m, _, _), (born, when) = state[k], modes[k], sp[k]
            tick, hwhen = birth_ticks(scheds[k]["spawn_time"], scheds[k]["chain"], t0[k], dts[k], T)
            assert np.array_equal(born, tick < T), f"scene {k}: births"
            assert np.array_equal(when.view(np.uint32), hwhen.view(np.uint32)), f"scene {k}: birth clocks"
            late += int(((tick > 0) & (tick < T)).sum())
            assert np.isfinite(loc).all() and np.isfinite(vel).all(), f"scene {k}"
            assert np.array_equal(m == MODE_UNBORN, ~born), f"scene {k}"
            ghost = (m == MODE_UNBORN) | (m == GONE)
            for i in np.nonzero(ghost)[0]:
                assert np.array_equal(loc[i, :2], _parked(i)) and not vel[i].any(), f"scene {k} ghost {i}"
            home = np.abs(scenes[k]["loc"][:, :2]).max() + 100.0
            assert (np.abs(loc[~ghost, :2]) < home).all() and (np.linalg.norm(vel[~ghost], axis=1) < 20.0).all(), f"scene {k}: bounded"
        assert late > B * 64 // 8, late
    finally:
        b.close()
