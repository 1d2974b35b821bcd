"""Sharded ticks at 4 and 8 ranks on one GPU, pinned to the oracle.

``_shards.ShardReplay`` replays what G ranks of ShardedStepper do -- G handles, rank blocks (``stepper.block_layout``), the exchange
of every packed() buffer ({z, vz} included), re-packs every 4 ticks with boundaries re-balanced from each rank's work() -- beside one
whole-crowd handle with the same partition.  Every tick the merged state is held to the oracle (v', x', waypoints, draw counters),
every rank's vehicles to every other rank's, the whole-crowd handle's and the host twin, and the shards to the whole-crowd handle
(bit for bit with the ordered kernel: results never depend on the packing).  The last test runs the real ShardedStepper in
G processes over gloo."""
import os
import socket

import numpy as np
import pytest

import _parity as P
import _shards as S
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd.config import default_sfm_config
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

TICKS = 12


def _c5_scene(n=6000, seed=5005):
    """c5 in miniature: all five forces, borders, static obstacles, vehicles that move on the device"""
    return scenarios.make_scenario(n, seed, n_borders=30, n_static=16, n_dynamic=12, border_len=(5.0, 25.0))


def _z3_scene(n=4200, seed=4201):
    """3-D, per-pedestrian radii in use, a crossing mask (some pedestrians feel no border force)"""
    sc = scenarios.make_scenario(n, seed, n_borders=20, n_static=10, n_dynamic=6, z_spread=1.5, border_len=(5.0, 25.0),
                                 modes=np.where(np.arange(n) % 7 == 3, 2, 1))
    sc.radius = np.float32(np.random.default_rng(seed).uniform(0.2, 0.45, n)).astype(np.float64)
    return sc


def _small_scene():
    return scenarios.make_scenario(300, 3003, n_borders=6, n_static=4, n_dynamic=8, border_len=(5.0, 20.0))


def _config(use_radius=False):
    cfg = default_sfm_config(scenarios.ALL_FORCES)
    cfg["use_ped_radius"] = use_radius
    return cfg


def _env(monkeypatch, ordered, geo_launch=False):
    """``geo_launch``: SFM_PAIR_GEO=0, the border / obstacle forces in a launch of their own instead of inside the pair launch -- the
    form in which a shard launches the next tick's geometry forces ahead, beside the exchange (tick_carry)"""
    env = {"SFM_CUTOFF": "1", "SFM_RESORT_EVERY": "0"}
    env.update({"SFM_SYM": "0", "SFM_IPW": "4", "SFM_TEAM": "1"} if ordered else {"SFM_SYM": "1"})
    if geo_launch:
        env["SFM_PAIR_GEO"] = "0"
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _check_vehicles(rep, sc, k):
    """every rank's vehicles -- the ranks without rows included -- bit for bit alike, like the whole-crowd handle's and the host twin's
    (scenarios.advance_dynamic); the host twin within fp32 of the oracle's float64 ring"""
    ranks = rep.vehicles()
    ref = rep.whole.engine.dynamic_obstacles()
    assert len(ref) == len(sc.dynamic_obstacles) > 0
    for r, got in enumerate(ranks):
        for (c_r, p_r), (c_w, p_w) in zip(got, ref):
            assert np.array_equal(c_r, c_w) and np.array_equal(p_r, p_w), f"rank {r}'s vehicles differ at tick {k}"
    for j, ((c_d, r_d), (c_h, r_h)) in enumerate(zip(ref, sc.dynamic_obstacles)):
        assert np.array_equal(c_d, c_h) and np.array_equal(r_d, r_h), f"vehicle {j} differs from the host twin at tick {k}"
        want = O.ellipse_ring(c_h, sc.dynamic_yaw[j], *sc.dynamic_extent[j])
        assert np.max(np.abs(r_d - want)) <= 4e-6 * max(1.0, np.abs(want).max()), f"vehicle {j} ring at tick {k}"


def _geometry_launched_ahead(rep):
    """Whether every rank took the geometry forces of its ticks from the launch its previous tick made ahead (tick_carry).  Such a tick
    makes one launch fewer than a tick right after set_shard, which drops what was launched ahead and launches the geometry itself;
    ticks of either kind make the same count as others of their kind."""
    fresh = [t for t, f in enumerate(rep.after_set_shard) if f]
    carried = [t for t, f in enumerate(rep.after_set_shard) if not f]
    assert fresh and carried
    for r in range(rep.world):
        a = {rep.launches[t][r] for t in fresh}
        b = {rep.launches[t][r] for t in carried}
        if len(a) != 1 or len(b) != 1 or a.pop() != b.pop() + 1:
            return False
    return True


def _no_launch_ahead(rep):
    """every tick of every rank made the same number of launches: nothing was launched ahead of a tick"""
    return all(len({l[r] for l in rep.launches}) == 1 for r in range(rep.world))


def _run_against_oracle(cfg, sc, world, layout, ordered, ticks=TICKS):
    """ShardReplay of ``ticks`` ticks, every tick checked -- with vehicles through the conditioned bound, which at most
    max(2, N // 100) rows of a tick may need (the budget of the handle's dynamic-obstacle tests).  Returns ([worst |dv'| / |v'| over
    all rows, over the rows without an exposure], rows that leaned on the conditioning, rows compared, the replay (closed))."""
    prm = O.OracleParams.from_config(cfg)
    crossing = (sc.mode == 2) | (sc.mode == 3)
    vehicles = len(sc.dynamic_obstacles) > 0
    rep = S.ShardReplay(cfg, sc, world, layout)
    n = rep.n
    loc, vel, wp = sc.loc.copy(), sc.vel.copy(), sc.waypoint.copy()
    draws = np.zeros(n, dtype=np.int64)
    worst, leaned, compared = [0.0, 0.0], 0, 0          # worst |dv'| / |v'| over all rows, over the rows without an exposure
    try:
        for k in range(ticks):
            seen = rep.ranks[0].engine.dynamic_obstacles()          # the vehicles this tick sees
            v_ref, expo, absum, wp_ref, dr_ref = S.oracle_tick(loc, vel, wp, draws, sc, seen, crossing, prm)
            rep.tick()
            dloc, dvel, dwp, ddr = rep.merged()
            if vehicles:
                needed = P.check_velocity_conditioned(dvel, v_ref, expo, absum, S.DT)
                assert needed <= max(2, n // 100), f"tick {k}: {needed} rows needed the conditioned bound"
                leaned += needed
            else:
                P.check_velocity(dvel, v_ref, expo, S.DT)
            compared += n
            rel = np.linalg.norm(dvel - v_ref, axis=1) / np.maximum(np.linalg.norm(v_ref, axis=1), 1e-12)
            worst = [max(worst[0], float(rel.max())), max(worst[1], float(rel[expo == 0].max(initial=0.0)))]
            # x' = fp32(x + dt v'), to one unit in the last place
            x_ref = loc + np.float64(np.float32(S.DT)) * dvel
            ulp = np.spacing(np.abs(x_ref).astype(np.float32)).astype(np.float64)
            assert (np.abs(dloc - x_ref) <= ulp).all(), f"x' at tick {k}: worst {np.max(np.abs(dloc - x_ref) / ulp):.2f} ulp"
            # waypoints and draw counters exactly; arrivals within fp32 noise of the threshold left out
            sure = np.abs(np.linalg.norm(wp[:, :2] - loc[:, :2], axis=1) - S.ARRIVE) > 1e-4
            assert np.array_equal(dwp[sure], wp_ref[sure, :2]), f"waypoints at tick {k}"
            assert np.array_equal(ddr[sure].astype(np.int64), dr_ref[sure]), f"draw counters at tick {k}"
            if vehicles:
                scenarios.advance_dynamic(sc, S.DT)
                _check_vehicles(rep, sc, k)
            wl, wv, ww, wd = rep.whole_state()
            if ordered:                                              # the packing never changes a result
                for a, b, what in ((dloc, wl, "x"), (dvel, wv, "v"), (dwp, ww, "waypoints")):
                    assert np.array_equal(a, b), f"{what} differ from the whole-crowd handle at tick {k}"
                assert np.array_equal(ddr, wd)
            else:                                                    # pairs across a boundary are summed in another order
                assert np.allclose(dloc, wl, rtol=2e-5, atol=2e-5) and np.allclose(dvel, wv, rtol=2e-5, atol=2e-5), f"tick {k}"
            loc, vel = dloc, dvel
            wp = np.concatenate([dwp, np.zeros((n, 1))], axis=1)
            draws = ddr.astype(np.int64)
        assert rep.repacks == (ticks - 1) // rep.resort_every
        return worst, leaned, compared, rep
    finally:
        rep.close()


@pytest.mark.parametrize("world,layout,geo_launch", [(4, (2, 2), False), (8, (2, 4), False), (8, (8, 1), False), (4, (2, 2), True)],
                         ids=["4_2x2", "8_2x4", "8_8x1", "4_2x2_geometry_ahead"])
def test_c5_shaped_shards_pinned_to_the_oracle(world, layout, geo_launch, monkeypatch):
    """Symmetric kernel on rank blocks (gx > 1 except for the slabs), vehicles on every shard, balanced unequal shares from the second
    re-pack on.  By default the border / obstacle workgroups ride in each tick's pair launch; ``geometry_ahead`` (SFM_PAIR_GEO=0) gives
    them a launch of their own, which a shard makes for the NEXT tick at the end of a tick, beside the exchange -- shown by the launch
    counts."""
    _env(monkeypatch, ordered=False, geo_launch=geo_launch)
    from carla_social_force_model_amd.stepper import block_layout
    if world == 8 and layout == (2, 4):
        assert block_layout(8) == layout                          # what bench.py --gpus 8 runs
    cfg = _config()
    worst, leaned, compared, rep = _run_against_oracle(cfg, _c5_scene(), world, layout, ordered=False)
    assert all("sym" in v for v in rep.variants()), rep.variants()
    assert rep.bounds_moved
    assert _geometry_launched_ahead(rep) if geo_launch else _no_launch_ahead(rep), rep.launches
    print(f"\nc5-shaped, G={world} {layout[0]}x{layout[1]}{' geometry ahead' if geo_launch else ''}: {rep.variants()[0]}, "
          f"launches per tick {[l[0] for l in rep.launches]}; worst |dv'|/|v'| {worst[0]:.3g} ({worst[1]:.3g} without exposure), "
          f"{leaned} of {compared} rows on the conditioned bound; bounds {rep.bounds}")


def test_c5_shaped_shards_with_the_ordered_kernel_equal_the_whole_crowd(monkeypatch):
    """SFM_SYM=0: every rank's rows are summed as the whole-crowd handle sums them, so G = 4 blocks equal it bit for bit over all
    ticks and re-packs (the ordered kernel measures no work: the replay moves the bounds by a lopsided cost)."""
    _env(monkeypatch, ordered=True)
    cfg = _config()
    worst, leaned, compared, rep = _run_against_oracle(cfg, _c5_scene(), 4, (2, 2), ordered=True)
    assert all(v.startswith("sfm_tick_kernel<4,false,false,1>") for v in rep.variants()), rep.variants()
    assert rep.bounds_moved
    print(f"\nc5-shaped ordered, G=4 2x2: worst |dv'|/|v'| {worst[0]:.3g} ({worst[1]:.3g} without exposure); bounds {rep.bounds}")


@pytest.mark.parametrize("world", [4, 8])
def test_3d_shards_pinned_to_the_oracle(world, monkeypatch):
    """N = 4200, n_pad = 4352: n_pad / 8 is not a whole number of tiles, so shares are unequal from tick 0.  3-D ({z, vz} goes
    through the exchange), radii and a crossing mask on, all forces; the ordered kernel over the kept tiles, bit for bit like the
    whole-crowd handle."""
    _env(monkeypatch, ordered=True)
    cfg = _config(use_radius=True)
    sc = _z3_scene()
    from carla_social_force_model_amd.stepper import equal_bounds
    eq = equal_bounds(sc.n, 4352, world)
    if world == 8:
        assert len({eq[r + 1] - eq[r] for r in range(world)}) > 1
    worst, leaned, compared, rep = _run_against_oracle(cfg, sc, world, None, ordered=True)
    assert all(v.startswith("sfm_tick_kernel<4,true,true,1>") for v in rep.variants()), rep.variants()
    assert rep.bounds_moved
    print(f"\n3-D, G={world}: worst |dv'|/|v'| {worst[0]:.3g} ({worst[1]:.3g} without exposure), {leaned} of {compared} rows on the conditioned bound")


def test_ranks_without_rows_move_their_vehicles(monkeypatch):
    """N = 300 on 8 ranks: ranks 4-6 own no rows and still advance their copy of the vehicles every tick."""
    _env(monkeypatch, ordered=False)
    cfg = _config()
    sc = _small_scene()
    from carla_social_force_model_amd.stepper import equal_bounds
    eq = equal_bounds(sc.n, 512, 8)
    assert sum(eq[r + 1] == eq[r] for r in range(8)) >= 2
    worst, leaned, compared, rep = _run_against_oracle(cfg, sc, 8, None, ordered=False)
    empty = [rep.bounds[r + 1] == rep.bounds[r] for r in range(8)]
    assert any(empty), rep.bounds
    # ranks with rows take the symmetric kernel; a rank without rows plans the ordered kernel and has no rows to run it on
    for r, v in enumerate(rep.variants()):
        assert ("sym" in v) != empty[r], (r, v, rep.bounds)
    print(f"\nN=300 on 8 ranks: worst |dv'|/|v'| {worst[0]:.3g} ({worst[1]:.3g} without exposure); bounds {rep.bounds}")


@pytest.mark.parametrize("geo_launch", [False, True], ids=["geometry_in_pair_launch", "geometry_ahead"])
def test_split_tick_equals_the_plain_tick_at_four_ranks(geo_launch, monkeypatch):
    """begin() / exchange / end() against run(1), G = 4 blocks with vehicles and geometry: the same bits every tick (DESIGN.md
    section 6), re-packs and moved bounds included.  ``geometry_ahead`` (SFM_PAIR_GEO=0): in both forms every tick's geometry forces
    come from the launch the previous tick made ahead, except right after set_shard."""
    _env(monkeypatch, ordered=False, geo_launch=geo_launch)
    cfg = _config()
    states, variants, ahead = [], [], []
    for split in (False, True):
        rep = S.ShardReplay(cfg, _c5_scene(), 4, (2, 2), split=split, whole=False)
        try:
            run = []
            for _ in range(TICKS):
                rep.tick()
                run.append(rep.merged() + (rep.vehicles(),))
            states.append(run)
            variants.append(rep.variants())
            ahead.append(_geometry_launched_ahead(rep) if geo_launch else _no_launch_ahead(rep))
            assert rep.bounds_moved
        finally:
            rep.close()
    for k, (a, b) in enumerate(zip(*states)):
        for x, y in zip(a[:4], b[:4]):
            assert np.array_equal(x, y), f"split tick differs at tick {k}"
        for va, vb in zip(a[4], b[4]):
            for (ca, pa), (cb, pb) in zip(va, vb):
                assert np.array_equal(ca, cb) and np.array_equal(pa, pb)
    assert all("sym" in v and "own|remote" not in v for v in variants[0]), variants[0]
    assert all("own|remote" in v for v in variants[1]), variants[1]
    assert ahead == [True, True]


# ---- the real stepper, G processes over gloo ----------------------------------------------------------------------
def _gloo_scene(kind):
    return (_c5_scene(), _config()) if kind == "c5" else (_z3_scene(), _config(use_radius=True))


def _gloo_worker(rank, world, port, out, kind, layout, split, ticks, every):
    import torch.distributed as dist
    from carla_social_force_model_amd.stepper import HipShardEngine, ShardedStepper
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SFM_CUTOFF="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sc, cfg = _gloo_scene(kind)
        eng = HipShardEngine(cfg, S.DT, device=0)
        st = ShardedStepper(eng, sc, rank=rank, world=world, resort_every=every, layout=layout, split=split)
        st.step(1)
        first = st.gather_state()
        st.step(ticks - 2)
        pre = st.gather_state()                     # the state the last tick starts from
        st.step(1)
        eng.synchronize()
        variant = eng.engine.kernel_variant()
        loc, vel, wp = st.gather_state()
        # one more re-pack of the final state (every rank holds all of it): the rows must come out in pack_order for the bounds the
        # stepper has set -- set_bounds hands them to set_partition
        st._gather(eng.row_data())
        eng.resort()
        eng.synchronize()
        rows = S.packed_rows(eng, st.n)
        if rank == 0:
            np.savez(out, loc1=first[0], vel1=first[1], wp1=first[2], loc_pre=pre[0], vel_pre=pre[1], wp_pre=pre[2], loc=loc, vel=vel,
                     wp=wp, rows=rows, bounds=np.array(st.bounds), n_pad=st.n_pad, variant=np.array(variant))
        eng.close()
    finally:
        dist.destroy_process_group()


def _check_gloo_tick(loc, vel, wp, vel_new, loc_new, sc, prm, what):
    """one tick of the gathered state against the oracle: v' (conditioned bound, the per-tick row budget), x' to one ulp"""
    n = sc.n
    crossing = (sc.mode == 2) | (sc.mode == 3)
    wp3 = np.concatenate([wp[:, :2], np.zeros((n, 1))], axis=1)
    v_ref, expo, absum, wp_ref, _ = S.oracle_tick(loc, vel, wp3, np.zeros(n, np.int64), sc, list(sc.dynamic_obstacles), crossing, prm)
    leaned = P.check_velocity_conditioned(vel_new, v_ref, expo, absum, S.DT)
    assert leaned <= max(2, n // 100), (what, leaned)
    x_ref = loc + np.float64(np.float32(S.DT)) * vel_new
    assert (np.abs(loc_new - x_ref) <= np.spacing(np.abs(x_ref).astype(np.float32)).astype(np.float64)).all(), what
    rel = np.linalg.norm(vel_new - v_ref, axis=1) / np.maximum(np.linalg.norm(v_ref, axis=1), 1e-12)
    return float(rel.max()), float(rel[expo == 0].max(initial=0.0)), leaned, wp_ref


@pytest.mark.parametrize("world,layout,kind", [(4, (2, 2), "c5"), (8, (2, 4), "c5"), (4, (2, 2), "3d")], ids=["4_2x2", "8_2x4", "4_2x2_3d"])
def test_sharded_stepper_over_gloo_pinned_to_the_oracle(world, layout, kind, tmp_path, monkeypatch):
    """ShardedStepper + HipShardEngine in G processes on the one GPU, split=True and split=False (the same bits), balance on, two
    re-packs in 20 ticks (unequal shares through the staging exchange).  Ticks 1 and 20 against the oracle (tick 20 from the gathered
    state of tick 19: every buffer the stepper exchanges -- {z, vz} of the 3-D crowd included -- must have reached every rank); tick 20
    against one process stepping the whole crowd."""
    import torch.multiprocessing as mp
    from carla_social_force_model_amd.stepper import HipShardEngine, ShardedStepper, equal_bounds
    ticks, every = 20, 8
    got = {}
    for split in (True, False):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        out = str(tmp_path / f"g{world}_{split}.npz")
        mp.spawn(_gloo_worker, args=(world, port, out, kind, layout, split, ticks, every), nprocs=world, join=True)
        got[split] = np.load(out)
    a, b = got[True], got[False]
    for key in ("loc1", "vel1", "wp1", "loc_pre", "vel_pre", "wp_pre", "loc", "vel", "wp", "rows", "bounds"):
        assert np.array_equal(a[key], b[key]), f"split and plain tick differ in {key}"
    assert "own|remote" in str(a["variant"]) and "sym" in str(b["variant"]) and "own|remote" not in str(b["variant"])
    sc, cfg = _gloo_scene(kind)
    n, n_pad = sc.n, int(a["n_pad"])
    bounds = [int(v) for v in a["bounds"]]
    assert bounds != equal_bounds(n, n_pad, world)                    # balanced: the shares are unequal
    # ticks 1 and 20 against the oracle
    prm = O.OracleParams.from_config(cfg)
    worst1, worst1_plain, leaned1, wp_ref = _check_gloo_tick(sc.loc, sc.vel, sc.waypoint, a["vel1"], a["loc1"], sc, prm, "tick 1")
    sure = np.abs(np.linalg.norm(sc.waypoint[:, :2] - sc.loc[:, :2], axis=1) - S.ARRIVE) > 1e-4
    assert np.array_equal(a["wp1"][sure], wp_ref[sure, :2])
    late = _gloo_scene(kind)[0]
    for _ in range(ticks - 1):                                            # the vehicles tick 20 sees
        scenarios.advance_dynamic(late, S.DT)
    worst20, worst20_plain, leaned20, _ = _check_gloo_tick(a["loc_pre"], a["vel_pre"], a["wp_pre"], a["vel"], a["loc"], late, prm,
                                                           "tick 20")
    # the final re-pack in pack_order of the final state, cut at the stepper's bounds
    order = S.rows_order(a["rows"][:, :2], a["loc"][:, :2])
    want = S.pack_order(a["loc"][:, 0], a["loc"][:, 1], n_pad, layout, bounds, aspect=S.crowd_aspect(sc.loc[:, 0], sc.loc[:, 1]))
    assert np.array_equal(order, want), f"{int((order != want).sum())} rows out of pack_order"
    # tick 20 against one process stepping the whole crowd
    monkeypatch.setenv("SFM_CUTOFF", "1")
    monkeypatch.setenv("SFM_RESORT_EVERY", str(every))
    eng = HipShardEngine(cfg, S.DT, device=0)
    try:
        st = ShardedStepper(eng, _gloo_scene(kind)[0])
        st.step(ticks)
        loc, vel, wp = st.gather_state()
    finally:
        eng.close()
    assert np.allclose(a["loc"], loc, rtol=2e-5, atol=2e-5) and np.allclose(a["vel"], vel, rtol=2e-5, atol=2e-5)
    assert np.array_equal(a["wp"], wp)
    print(f"\ngloo {kind} G={world} {layout[0]}x{layout[1]}: worst |dv'|/|v'| tick 1 {worst1:.3g} ({worst1_plain:.3g} without exposure, "
          f"{leaned1} rows conditioned), tick 20 {worst20:.3g} ({worst20_plain:.3g}, {leaned20}); bounds {bounds}")
