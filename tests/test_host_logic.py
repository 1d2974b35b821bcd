"""CPU tests of the host-side mirror of the reference interface: mode FSM, PedState layout and accessors,
config reading (bug-compatible), gap acceptance, geometry/scenario generators, shard arithmetic."""
import numpy as np
import pytest

from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd.check_traffic import check_traffic
from carla_social_force_model_amd.config import default_sfm_config, load_sfm_config
from carla_social_force_model_amd.engine import params_from_config
from carla_social_force_model_amd.ped_mode_manager import PedMode, PedModeManager
from carla_social_force_model_amd.pedestrian_state import PED_STATE_DTYPE, PedState
from carla_social_force_model_amd.stepper import shard_bounds


def test_record_layout_is_the_reference_layout():
    dt = np.dtype(PED_STATE_DTYPE)
    assert dt.itemsize == 132
    assert {k: dt.fields[k][1] for k in dt.names} == {'name': 0, 'id': 32, 'loc': 36, 'vel': 60, 'next_waypoint': 84,
                                                      'mode': 108, 'radius': 116, 'target_speed': 124}


def test_mode_fsm_transitions():
    m = PedModeManager("p", 1.2, PedMode.WALKING_SIDEWALK, 1.5, 1.0)
    assert m.target_speed == 1.2 and m.crossing_speed == pytest.approx(1.8)
    m.set_mode(PedMode.CROSSING_ROAD)                 # diverted: look first
    assert m.current_mode == PedMode.CHECKING_TRAFFIC and m.target_speed == 0
    m.set_mode(PedMode.CROSSING_ROAD)
    assert m.current_mode == PedMode.CROSSING_ROAD and m.target_speed == pytest.approx(1.8)
    m.set_mode(PedMode.WALKING_SIDEWALK)              # diverted: still on the road, keeps crossing speed
    assert m.current_mode == PedMode.ROAD_TO_SIDEWALK and m.target_speed == pytest.approx(1.8)
    m.set_mode(PedMode.WALKING_SIDEWALK)
    assert m.current_mode == PedMode.WALKING_SIDEWALK and m.target_speed == 1.2
    m.tick(10.0)
    m.set_mode(PedMode.IDLE)
    assert m.target_speed == 0 and m.next_mode_time == 15.0
    m.tick(14.9)
    assert m.current_mode == PedMode.IDLE
    m.tick(15.0)
    assert m.current_mode == PedMode.WALKING_SIDEWALK and m.target_speed == 1.2
    # the constructor does not run the initial mode's entry action
    assert PedModeManager("q", 1.0, PedMode.IDLE, 1.5, 1.0).target_speed == 1.0


def test_mode_fsm_replays_the_reference_trace():
    """tests/golden/fsm_trace.npz: 400 scripted tick / set_mode calls replayed on the REFERENCE's PedModeManager
    (tests/golden/make_golden_fsm.py); the mirror must land in the same (mode, target_speed, next_mode_time)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fsm_trace.npz"))
    objs = [PedModeManager(f"p{k}", float(a), PedMode(int(b)), float(c), float(d)) for k, (a, b, c, d) in enumerate(z["init"])]
    for (k, op, arg), (mode, target, nxt) in zip(z["script"], z["trace"]):
        o = objs[int(k)]
        if op == 0:
            o.tick(float(arg))
        else:
            o.set_mode(PedMode(int(arg)))
        assert (int(o.current_mode), o.target_speed, o.next_mode_time) == (int(mode), target, nxt)


def _ped(i, mode=PedMode.WALKING_SIDEWALK):
    mm = PedModeManager(f"ped_{i}", 1.0 + 0.1 * i, mode, 1.5, 1.5)
    return (f"ped_{i}", 100 + i, [i, 2.0 * i, 0.0], [0.1, 0.2, 0.0], [10.0, 10.0, 0.0], mm, 0.3, 1.0 + 0.1 * i)


def test_pedstate_bookkeeping():
    ps = PedState({})
    assert ps.state is None and ps.max_speed_factor == 1.3
    for i in range(40):                                # crosses the growth boundary
        ps.add_pedestrian(_ped(i))
    assert ps.size() == 40 and ps.state.dtype.itemsize == 132
    assert np.allclose(ps.loc()[7], [7, 14, 0]) and ps.walker_id()[7] == 107 and ps.name()[7] == "ped_7"
    ps.update_state(107, [1.0, 1.0, 0.5], [0.0, 0.0, 0.0])
    assert np.allclose(ps.loc()[7], [1, 1, 0.5]) and np.allclose(ps.speeds()[7], 0)
    ps.update_next_waypoint("ped_3", ([5.0, 5.0, 0.0], True))
    assert ps.mode()[3].current_mode == PedMode.CHECKING_TRAFFIC
    ps.apply_current_mode()
    assert ps.target_speed()[3] == 0 and ps.target_speed()[4] == pytest.approx(1.4)
    assert np.allclose(ps.max_speed(), 1.3 * ps.target_speed())
    ps.mode()[5].set_mode(PedMode.CROSSING_ROAD); ps.mode()[5].set_mode(PedMode.CROSSING_ROAD)
    assert ps.crossing_mask().sum() == 1 and ps.crossing_mask()[5]
    ps.remove_pedestrian("ped_0")
    assert ps.size() == 39 and ps.name()[0] == "ped_1"
    with pytest.raises(IndexError):
        ps.update_next_waypoint("nobody", ([0, 0, 0], False))
    d = ps.desired_directions()
    assert d.shape == (39, 3) and np.allclose(np.linalg.norm(d[:, :2], axis=1), 1) and np.all(d[:, 2] == 0)
    ps.record_current_state(0.5)
    snap = ps.get_all_states()[0.5]
    assert snap['mode'][4] == PedMode.CROSSING_ROAD and snap.shape == (39,)
    view = ps.state[['id', 'vel']]                     # the get_new_velocities view writes through
    view['vel'] = np.ones((39, 3))
    assert np.all(ps.vel() == 1.0)
    loc, vel, wp, ts, rad, cm = ps.numeric_columns()
    assert loc.flags['C_CONTIGUOUS'] and loc.shape == (39, 3) and cm.dtype == bool


def test_config_surface_and_bug_compat():
    cfg = load_sfm_config()
    assert cfg == default_sfm_config()
    p = params_from_config(cfg, 0.05)
    assert p.tau == 0.5 and p.max_speed_factor == pytest.approx(1.3) and list(p.enabled) == [1] * 5
    assert p.pedestrian.A == 4.5 and p.static_obstacle.A == 15 and p.dynamic_obstacle.perception_threshold == 50
    assert p.border_a == 6.0 and p.border_b == pytest.approx(0.3)
    cfg["acceleration_force"]["tau"] = 0.9
    cfg["max_speed_multiplier"] = 2.0
    assert params_from_config(cfg, 0.05).tau == 0.5                        # file key ignored, like the reference
    q = params_from_config(cfg, 0.05, honour_file_keys=True)                # documented opt-in
    assert q.tau == pytest.approx(0.9) and q.max_speed_factor == 2.0
    cfg["goal_force"] = {"tau": 0.25}
    assert params_from_config(cfg, 0.05).tau == 0.25
    bad = default_sfm_config()
    del bad["pedestrian_force"]
    with pytest.raises(KeyError):
        params_from_config(bad, 0.05)
    bad = default_sfm_config()
    bad["forces"]["ped_repulsive_force"] = True
    with pytest.raises(AttributeError):
        params_from_config(bad, 0.05)
    bad = default_sfm_config()
    bad["border_force"] = {}
    p = params_from_config(bad, 0.05)
    assert p.border_a == 3.0 and p.border_b == pytest.approx(0.1)           # code-side defaults (forces.py:135-136)


def test_check_traffic_closed_form():
    mm = PedModeManager("p", 1.0, PedMode.WALKING_SIDEWALK, 1.5, 1.0)        # crossing speed 1.5, margin 1 s
    ped = {"loc": np.array([0.0, -3.0, 0.0]), "next_waypoint": np.array([0.0, 3.0, 0.0]), "mode": mm}
    ring = np.zeros((6, 2))
    ext = [np.array([2.0, 1.0])]
    # vehicle far to the left, driving right at 10 m/s: reaches x=0 after ~2 s, pedestrian is there at 2 s -> wait
    assert check_traffic(ped, [(np.array([-22.0, 0.0]), ring)], [np.array([10.0, 0.0])], ext) is False
    # same vehicle driving away -> no intersection -> go
    assert check_traffic(ped, [(np.array([-22.0, 0.0]), ring)], [np.array([-10.0, 0.0])], ext) is True
    # stationary vehicle on the path: intersection exists but speed 0 is skipped (check_traffic.py:49)
    assert check_traffic(ped, [(np.array([0.0, 0.0]), ring)], [np.array([0.0, 0.0])], ext) is True
    # vehicle passes long before the pedestrian arrives
    assert check_traffic(ped, [(np.array([-3.0, 0.0]), ring)], [np.array([30.0, 0.0])], ext) is True
    # negative safety margin: cross without looking
    mm.crossing_safety_margin = -1
    assert check_traffic(ped, [(np.array([-22.0, 0.0]), ring)], [np.array([10.0, 0.0])], ext) is True


def test_scenario_generators_follow_reference_formats():
    sc = scenarios.make_scenario(100, 3, n_borders=5, n_static=4, n_dynamic=3)
    assert sc.loc.shape == (100, 3) and np.all(sc.loc[:, 2] == 0)
    for a in (sc.loc, sc.vel, sc.waypoint, sc.target_speed):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))      # fp32-representable
    d = np.linalg.norm(sc.loc[:, None, :2] - sc.loc[None, :, :2], axis=-1) + np.eye(100)
    assert d.min() > 0.3                                                         # jittered grid: no coincident peds
    line, c, sl = scenarios.straight_border([0.0, 0.0], [10.0, 0.0])
    assert len(line) == 100 and np.allclose(c, line[50]) and sl == pytest.approx(10.0)
    ring = scenarios.ellipse_ring(np.array([0.0, 0.0]), 0.0, 2.4, 1.0)
    assert len(ring) == 68 and np.allclose(ring[0], [2.4 * np.sqrt(2), 0.0], atol=1e-6)
    assert len(scenarios.ellipse_ring(np.array([0.0, 0.0]), 0.3, 0.1, 0.1)) == 6
    info = sc.section_info()
    assert info.shape == (5, 2) and info.dtype == object
    sc2 = scenarios.make_scenario(100, 3, n_borders=5, n_static=4, n_dynamic=3)
    assert np.array_equal(sc.loc, sc2.loc) and np.array_equal(sc.borders[2], sc2.borders[2])
    for name, kw in scenarios.BASELINE_CONFIGS.items():
        assert kw["seed"] == 1000 + int(name[1])


def test_shard_bounds_cover_everything_once():
    for n, world in ((4096, 1), (4096, 8), (1000, 4), (65536, 4), (300, 2)):
        n_pad = -(-n // 256) * 256
        rows = []
        for r in range(world):
            lo, hi, chunk = shard_bounds(n, n_pad, r, world)
            assert chunk * world == n_pad and 0 <= lo <= hi <= n
            rows += list(range(lo, hi))
        assert rows == list(range(n))
    with pytest.raises(ValueError):
        shard_bounds(100, 256, 0, 3)


def test_balanced_bounds_evens_out_a_lopsided_cost():
    """stepper.balanced_bounds: boundaries move towards equal cost, stay whole tiles, never cross, never lose the ends."""
    from carla_social_force_model_amd.stepper import balanced_bounds, equal_bounds
    n = 262144
    b = equal_bounds(n, n, 8)
    density = lambda r: 1.0 if r in (0, 7) else 1.25            # interior ranks pay for two boundaries
    first = None
    for _ in range(6):
        costs = [(b[r + 1] - b[r]) * density(r) for r in range(8)]
        spread = max(costs) / (sum(costs) / 8)
        first = first or spread
        b = balanced_bounds(b, costs, n)
        assert b[0] == 0 and b[-1] == n and all(x % 64 == 0 for x in b) and all(b[r + 1] - b[r] >= 64 for r in range(8))
    assert first > 1.04 and spread < 1.005
    assert balanced_bounds([0, 128, 256], [0.0, 0.0], 256) == [0, 128, 256]     # no measure: boundaries stay
    assert balanced_bounds([0, 256], [5.0], 256) == [0, 256]


def test_interior_shard_bounds_are_whole_tiles_for_any_size():
    """sfm_set_partition (and the symmetric kernel's shards) only take interior bounds that are multiples of 64: the equal
    split and every re-balanced split must deliver that for odd crowd sizes and world sizes too (round-2 advisor finding:
    n = 520 on 4 ranks used to give [0, 192, 384, 520, 520], n_pad = 768 on 8 ranks 96-row chunks)."""
    from carla_social_force_model_amd.stepper import balanced_bounds, equal_bounds
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 200, 520, 700, 768, 1000, 4096, 4160, 10007, 65536):
        n_pad = (n + 255) // 256 * 256
        for world in (1, 2, 4, 8):
            b = equal_bounds(n, n_pad, world)
            assert len(b) == world + 1 and b[0] == 0 and b[-1] == n
            assert all(b[k] <= b[k + 1] for k in range(world)), (n, world, b)
            assert all(x % 64 == 0 for x in b[:-1]), (n, world, b)
            if (n_pad // world) % 64 == 0 and n == n_pad:
                assert b == [n_pad // world * r for r in range(world + 1)]       # the in-place all-gather's even split
            for _ in range(4):
                costs = [float(c) for c in rng.uniform(0.5, 2.0, world) * np.maximum(1, np.diff(b))]
                b = balanced_bounds(b, costs, n)
                assert len(b) == world + 1 and b[0] == 0 and b[-1] == n
                assert all(b[k] <= b[k + 1] for k in range(world)), (n, world, b)
                assert all(x % 64 == 0 for x in b[:-1]), (n, world, b)
    assert equal_bounds(520, 768, 4) == [0, 192, 384, 512, 520]
    assert balanced_bounds([0, 64, 128, 192, 200], [1.0, 1.0, 1.0, 30.0], 200) == [0, 64, 128, 192, 200]


def test_gap_acceptance_and_vehicle_rings_agree_with_the_oracles_restatement():
    """SURVEY.md section 8f rows 2 and 3.  Neither obstacles.py (carla) nor check_traffic.py (shapely) can run here and the
    reference holds no fixtures for them, so the product's host code is checked against an independent float64 restatement in
    oracle/ written from the reference source (the restatement itself is held to the reference's outputs in test_traffic_golden.py): 4000 random crossings incl. axis-aligned
    and collinear ones, and the ellipse rings of random vehicles."""
    from types import SimpleNamespace
    from carla_social_force_model_amd import scenarios
    from oracle import sfm_oracle as O
    rng = np.random.default_rng(2024)
    disagreements, waits = 0, 0
    for k in range(4000):
        m = int(rng.integers(1, 4))
        snap = (lambda a: np.round(a)) if k % 3 == 0 else (lambda a: a)          # every third case on the integer grid: collinear / touching paths happen
        loc, goal = snap(rng.uniform(-10, 10, 2)), snap(rng.uniform(-10, 10, 2))
        if (loc == goal).all():
            goal = goal + 1.0
        vlocs, vvels = [], []
        for _ in range(m):                                   # most vehicles are aimed at a point of the pedestrian's path
            if rng.random() < 0.7:
                tgt = loc + rng.uniform(0, 1) * (goal - loc)
                h = rng.uniform(0, 2 * np.pi)
                d = np.array([np.cos(h), np.sin(h)])
                sp = rng.uniform(2, 12)
                vlocs.append(snap(tgt - d * sp * rng.uniform(0, 8)))
                vvels.append(snap(d * sp) * (rng.random() > 0.1))
            else:
                vlocs.append(snap(rng.uniform(-30, 30, 2)))
                vvels.append(snap(rng.uniform(-12, 12, 2)) * (rng.random() > 0.1))
        exts = [rng.uniform(0.5, 2.5, 2) for _ in range(m)]
        speed, margin = float(rng.uniform(0.8, 2.0)), float(rng.choice([-1.0, 0.0, 0.5, 1.5]))
        ped = {'loc': np.append(loc, 0.0), 'next_waypoint': np.append(goal, 0.0),
               'mode': SimpleNamespace(crossing_speed=speed, crossing_safety_margin=margin)}
        got = check_traffic(ped, [(v, None) for v in vlocs], vvels, exts)
        want = O.gap_accepted(loc, goal, speed, margin, vlocs, vvels, exts)
        disagreements += got != want
        waits += not want
    assert disagreements == 0 and 200 < waits < 3800
    for _ in range(50):
        c, yaw, ex, ey = rng.uniform(-500, 500, 2), rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 3.0), rng.uniform(0.3, 1.5)
        want = O.ellipse_ring(c, yaw, ex, ey)
        local = scenarios.ring_local_offsets(ex, ey)
        got = scenarios.place_ring_f32(c, yaw, local)
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-4                                  # fp32 placement at |c| ~ 500 m: ulp 6e-5
        assert np.max(np.abs(scenarios.ellipse_ring(scenarios._f32(c), yaw, ex, ey) - want)) <= 1e-4


def test_block_layout_of_the_ranks():
    from carla_social_force_model_amd.stepper import block_layout
    assert [block_layout(w) for w in (1, 2, 3, 4, 6, 8)] == [(1, 1), (1, 2), (3, 1), (2, 2), (3, 2), (2, 4)]
    assert block_layout(8, (8, 1)) == (8, 1)
    with pytest.raises(ValueError):
        block_layout(4, (8, 1))


def test_bench_flags_counters_from_another_build_as_stale(tmp_path, monkeypatch):
    """bench.py's roofline multiplies committed PMC counters by a live launch time; the summary carries the git blob id of
    sfm_kernels.hip at collection time and the line must say `counters_stale` when the loaded build's source differs
    (round-2 verdict, bench hygiene).  The blob id is git's own (`git hash-object`), computed without a .git directory."""
    import hashlib
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    src = tmp_path / "kernels.hip"
    src.write_bytes(b"__global__ void k() {}\n")
    blob = hashlib.sha1(b"blob %d\0" % len(src.read_bytes()) + src.read_bytes()).hexdigest()
    assert bench.git_blob_sha1(str(src)) == blob
    assert bench.git_blob_sha1(str(tmp_path / "missing")) is None
    summary = tmp_path / "pmc.csv"
    summary.write_text(f"# rocprofv3 --pmc means per launch; sfm_kernels.hip git-blob {blob}\n"
                       "workload,kernel,counter,mean_per_launch,launches\nc2,sfm_fused_tick_kernel,SQ_INSTS_VALU,100.000,5\n")
    monkeypatch.setattr(bench, "PMC_SUMMARY", str(summary))
    monkeypatch.setattr(bench, "KERNEL_SOURCE", str(src))
    pmc, stamp = bench.pmc_counters("c2", "sfm_fused_tick_kernel")
    assert pmc == {"SQ_INSTS_VALU": 100.0} and stamp["counters_stale"] is False
    src.write_bytes(b"__global__ void k() { }\n")                    # the kernels were edited after the counter passes
    assert bench.pmc_counters("c2", "sfm_fused_tick_kernel")[1]["counters_stale"] is True
    assert bench.pmc_counters("c9", "nothing")[0] == {}
    # the committed summary belongs to the committed kernels
    monkeypatch.undo()
    pmc, stamp = bench.pmc_counters("c2", "sfm_fused_tick_kernel")
    assert "SQ_INSTS_VALU" in pmc and "VALU_PER_64_PAIR_STEP" in pmc and stamp["counters_stale"] is False


def test_bench_dump_outputs_keeps_float32_under_the_cap(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every array as DIR/<name>.npy in float32; above the size cap the same seeded, sorted sample of
    rows from each array, so two runs (two builds) stay comparable row for row."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(5)
    arrays = {"loc": rng.normal(size=(1000, 3)), "vel": rng.normal(size=(1000, 3)), "waypoint": rng.normal(size=(1000, 2))}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "all" / (k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, v.astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 4 * 100)             # room for 100 rows of 3 + 3 + 2 floats
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    total = 0
    for k, v in arrays.items():
        a, b = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert a.shape == (100, v.shape[1]) and np.array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    rows = [int(np.flatnonzero((arrays["loc"].astype(np.float32) == r).all(axis=1))[0]) for r in np.load(tmp_path / "a" / "loc.npy")]
    assert rows == sorted(rows)
    assert np.array_equal(np.load(tmp_path / "a" / "vel.npy"), arrays["vel"][rows].astype(np.float32))


def test_mode_caches_follow_every_way_a_mode_can_change():
    """Round 4: ``apply_current_mode`` / ``crossing_mask`` are cached arrays, rebuilt when a mode object says that something changed
    (ModeWatch.version).  Every way the reference's callers change a mode or a target speed must get through -- set_mode
    (pedestrian_state.py:88-92), the FSM's own tick (ped_mode_manager.py:30-35), a direct write to a manager's attribute, spawn and
    removal -- and a write into state['target_speed'] is overwritten at the next tick like in the reference (pedestrian_state.py:94-95).
    A mode object of another class (the reference's own PedModeManager) switches the caching off."""
    from carla_social_force_model_amd.host_state import PedState
    ps = PedState({})
    mgrs = [PedModeManager(f"p{i}", 1.0 + 0.1 * i, PedMode.WALKING_SIDEWALK, 1.5, 1.0) for i in range(5)]
    for i, m in enumerate(mgrs):
        ps.add_pedestrian((f"p{i}", i, np.zeros(3), np.zeros(3), np.ones(3), m, 0.3, 9.9))
    ps.apply_current_mode()
    assert np.allclose(ps.target_speed(), [1.0, 1.1, 1.2, 1.3, 1.4]) and not ps.crossing_mask().any()
    v0 = ps.watch.version
    ps.apply_current_mode()
    assert ps.watch.version == v0                                     # nothing changed: nothing rebuilt
    ps.state['target_speed'][2] = 7.0                                 # a caller's write is overwritten at the next tick
    ps.apply_current_mode()
    assert ps.target_speed()[2] == pytest.approx(1.2)
    ps.update_next_waypoint("p1", (np.array([5.0, 5.0, 0.0]), True))  # WALKING -> asked to cross -> CHECKING_TRAFFIC: stands still
    ps.apply_current_mode()
    assert ps.target_speed()[1] == 0 and mgrs[1] in ps.watch.checking and not ps.crossing_mask()[1]
    mgrs[1].set_mode(PedMode.CROSSING_ROAD)                           # gap accepted (pedestrian_simulation.py:70)
    ps.apply_current_mode()
    assert ps.target_speed()[1] == pytest.approx(1.5 * 1.1) and ps.crossing_mask()[1] and mgrs[1] not in ps.watch.checking
    mgrs[3].target_speed = 0.25                                       # a direct write to the mode object
    ps.apply_current_mode()
    assert ps.target_speed()[3] == 0.25
    # an IDLE pedestrian: only it is ticked one by one; it wakes up waiting_time after the WATCH's clock, not its own stale one
    ps.watch.sim_time = 12.0
    mgrs[4].set_mode(PedMode.IDLE)
    assert mgrs[4] in ps.watch.idle and mgrs[4].next_mode_time == 17.0
    ps.apply_current_mode()
    assert ps.target_speed()[4] == 0
    for m in tuple(ps.watch.idle):
        m.tick(16.9)
    assert mgrs[4].current_mode == PedMode.IDLE
    for m in tuple(ps.watch.idle):
        m.tick(17.0)
    ps.apply_current_mode()
    assert mgrs[4].current_mode == PedMode.WALKING_SIDEWALK and not ps.watch.idle and ps.target_speed()[4] == pytest.approx(1.4)
    ps.remove_pedestrian("p1")                                        # rows shift: the arrays follow
    ps.apply_current_mode()
    assert ps.size() == 4 and np.allclose(ps.target_speed(), [1.0, 1.2, 0.25, 1.4]) and not ps.crossing_mask().any()
    assert mgrs[1]._watch is None
    rows = ps.pack_rows(np.empty((8, 9), np.float32))
    assert rows.shape == (4, 9) and np.allclose(rows[:, 6], [1.0, 1.2, 0.25, 1.4]) and np.allclose(rows[:, 7], 0.3) and not rows[:, 8].any()

    class Foreign:                                                    # e.g. the reference's own class: no hooks, no caching
        def __init__(self):
            self.target_speed, self.current_mode = 0.9, PedMode.CROSSING_ROAD
    f = Foreign()
    ps.add_pedestrian(("px", 9, np.zeros(3), np.zeros(3), np.ones(3), f, 0.3, 0.0))
    ps.apply_current_mode()
    assert ps.target_speed()[-1] == 0.9 and ps.crossing_mask()[-1]
    f.target_speed, f.current_mode = 0.4, PedMode.WALKING_SIDEWALK   # a silent change is still seen: every tick re-reads the objects
    ps.apply_current_mode()
    assert ps.target_speed()[-1] == 0.4 and not ps.crossing_mask()[-1]
