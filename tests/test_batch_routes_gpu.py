"""GPU tests of the routes planned on the device (sfm_batch_set_routes, sfm_batch_plan_routes, sfm_batch_plan_routes_device,
sfm_batch_download_routes, SFM_BATCH_PTR_ROUTE_GOALS / _ROUTE_STATUS; SfmBatch.set_routes / plan_routes / plan_routes_device /
routes / route_goal_tensor / route_status_tensor).

Every comparison is bitwise against the NumPy twin route.plan_scene, which tests/test_batch_routes_host.py holds to the reference's
own planner.  Graphs of 1, 2, 63, 64, 65, 257 and 1 024 nodes (a chain of 1 024: 1 023 rounds, the round cap and termination; a
star; two components; the grid of exact ties; 257 nodes with more than 2 048 adjacency entries, which the kernel reads from global
memory, all the others from LDS), scenes of 1, 2, 5 and 300 rows (more rows than waves: a wave takes a second row).
Run on the MI355X box with  python -m pytest tests -m gpu."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import _route_cases as RC
import test_batch_modes_gpu as M
from carla_social_force_model_amd import route as R
from carla_social_force_model_amd._lib import SfmLibraryError, iptr
from carla_social_force_model_amd.batch import SfmBatch

pytestmark = pytest.mark.gpu

CAP = 16
SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3
f32 = lambda a: np.asarray(a, np.float32)


def _graphs():
    lone = {"nodes": [[1.0, 2.0]], "edges": np.zeros((0, 2), np.int64), "types": np.zeros(0, np.int64)}
    pair = {"nodes": [[0.0, 0.0], [7.0, 1.0]], "edges": [[0, 1]], "types": [RC.CROSSWALK]}
    return [lone, pair, RC.chain(63), RC.street_grid(8, 8, 31, spacing=6.0, jitter=1.5), RC.random_graph(65, 32), RC.star(257),
            RC.chain(1024), RC.two_components(), RC.integer_grid(6), None, RC.random_graph(257, 33, extra=4.5), RC.three_ways()]


ROWS = (1, 2, 5, 300, 5, 5, 2, 5, 5, 2, 5, 5)


@lru_cache(maxsize=None)
def _world(z3=False):
    """The scenes, their mode plans, graphs, graph types (0: not routed), goals (built once; nothing below changes them)."""
    graphs = _graphs()
    rng = np.random.default_rng(2323)
    scenes, plans, gts, goals = [], [], [], []
    for k, (n, g) in enumerate(zip(ROWS, graphs)):
        sc, plan, _ = M._scene(n, 2350 + k, 0, z_spread=1.5 if z3 else 0.0, borders=2)
        nodes = np.asarray(g["nodes"], np.float64) if g is not None else np.zeros((1, 2))
        sc["loc"][:, :2] = f32(nodes[rng.integers(0, len(nodes), n), :2] + rng.uniform(-2.5, 2.5, (n, 2))).astype(np.float64)
        gl = np.zeros((n, 3))
        gl[:, :2] = nodes[rng.integers(0, len(nodes), n), :2] + rng.uniform(-2.5, 2.5, (n, 2))
        gl[:, 2] = rng.uniform(-5, 5, n)                              # (z is ignored)
        gt = rng.integers(1, 4, n).astype(np.uint8)
        gt[rng.random(n) < 0.2] = 0                                    # rows outside the mask
        if k == 3:
            sc["loc"][7, :2] = [3.0e15, -3.0e15]                       # a ghost: status 4
            gl[9, 0] = np.nan                                          # status 5
            gl[11, 1] = np.inf
            gt[[7, 9, 11]] = 2
        if k == 6:                                                     # the chain of 1 024 from end to end: status 3, after 1 023 rounds
            sc["loc"][0, :2], gl[0, :2], gt[0] = [-1.0, 0.5], [3070.0, 0.5], 1
            sc["loc"][1, :2], gl[1, :2], gt[1] = [3040.0, 0.5], [3071.0, -0.5], 3     # ... and its last ten nodes: planned
        scenes.append(sc); plans.append(plan); gts.append(gt); goals.append(gl)
    return scenes, plans, graphs, gts, goals


def _batch(idx=None, z3=False, capacity=CAP, routes=True):
    scenes, plans, graphs, gts, goals = _world(z3)
    idx = range(len(scenes)) if idx is None else idx
    pick = lambda v: [v[k] for k in idx]
    b = SfmBatch([M._config(k) for k in idx], [0.05] * len(idx))
    try:
        b.upload(pick(scenes), planar=None if not z3 else False)
        b.set_modes(pick(plans), despawn_on_arrival=True, sim_time0=0.0, arrive_thresholds=2.0, scenes=pick(scenes))
        if routes:
            b.set_routes(pick(graphs), [np.maximum(g, 1) for g in pick(gts)], pick(goals), mask=[g != 0 for g in pick(gts)], capacity=capacity)
    except Exception:
        b.close()
        raise
    return b


def _read(b):
    """Everything a plan can change, per scene."""
    out = []
    for (loc, _), (wp, _), (m, t, c), r in zip(b.state(), b.waypoints(), b.modes(), b.routes()):
        out.append({"loc": loc, "wp": wp, "mode": m, "target": t, "cursor": c, **{k: r[k] for k in ("status", "s", "t", "L", "cost", "queue")}})
    return out


def _same_row(u, v, i):
    return all(np.array_equal(u[k][i], v[k][i]) for k in ("wp", "mode", "target", "cursor")) and \
        np.array_equal(u["queue"][i][0], v["queue"][i][0]) and np.array_equal(u["queue"][i][1], v["queue"][i][1])


def _check_scene(what, before, after, graph, gt, goals, initial, capacity=CAP, pos=None):
    """One scene after a plan against the twin planned from ``pos`` (default: where the rows stood before)."""
    pos = before["loc"] if pos is None else pos
    twin = R.plan_scene(R.pack_graph(graph), gt, pos, goals, capacity, modes=before["mode"])
    seen = set()
    for i, p in enumerate(twin):
        w = f"{what}, row {i}"
        if p is None:                                                  # not routed: untouched, queue and cursor included
            assert _same_row(before, after, i) and after["status"][i] == 0, w
            continue
        seen.add(p["status"])
        got = tuple(after[k][i] for k in ("status", "s", "t", "L"))
        assert got == (p["status"], p["s"], p["t"], p["L"]), (w, got, p["status"], p["s"], p["t"], p["L"])
        assert np.array_equal(after["cost"][i], p["cost"]), (w, after["cost"][i], p["cost"])
        if p["status"] in (R.STATUS_NOT_LIVE, R.STATUS_BAD_GOAL):      # left exactly as it was
            assert _same_row(before, after, i), w
            continue
        cursor, xy, cross = R.queue_slots(p, capacity)
        first = p["xy"][0] if p["status"] == R.STATUS_PLANNED else f32(goals[i][:2])
        assert np.array_equal(after["wp"][i], first), (w, after["wp"][i], first)
        assert after["mode"][i] == 1 and after["target"][i] == np.float32(initial[i]) and after["cursor"][i] == cursor, w
        qxy, qc = after["queue"][i]
        assert len(qxy) == capacity and np.array_equal(qxy[cursor:], xy) and np.array_equal(qc[cursor:], cross), w
    return seen


def _check_all(what, b, before, after, idx=None, pos=None, only=None):
    scenes, plans, graphs, gts, goals = _world(not b.planar)
    idx = list(range(len(scenes)) if idx is None else idx)
    seen = set()
    for j, k in enumerate(idx):
        if only is not None and not only[j]:
            continue
        seen |= _check_scene(f"{what}: scene {k}", before[j], after[j], graphs[k], gts[k], goals[k], plans[k]["initial_speed"],
                             pos=None if pos is None else pos[j])
    return seen


@pytest.fixture(scope="module")
def crowd():
    """The whole batch planned once: (before, after).  Shared, never changed."""
    b = _batch()
    try:
        before = _read(b)
        b.plan_routes()
        return before, _read(b)
    finally:
        b.close()


def test_every_shape_equals_the_twin_and_every_status_is_met(crowd):
    before, after = crowd
    seen = _check_all("crowd", SimpleBatchView(True), before, after)
    assert seen == {1, 2, 3, 4, 5}
    # the chain of 1 024: found end to end (1 023 rounds), too long for any queue
    assert (after[6]["status"][0], after[6]["s"][0], after[6]["t"][0], after[6]["L"][0]) == (3, 0, 1023, 1025)
    assert after[6]["cost"][0] == np.float32(3069.0) and after[6]["status"][1] == 1


class SimpleBatchView:
    def __init__(self, planar):
        self.planar = planar


@pytest.mark.parametrize("k", range(len(ROWS)))
def test_a_scene_alone_equals_the_scene_in_the_crowd(crowd, k):
    b = _batch([k])
    try:
        b.plan_routes()
        alone = _read(b)[0]
    finally:
        b.close()
    for key, v in crowd[1][k].items():
        if key == "queue":
            assert all(np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) for a, c in zip(alone[key], v)), key
        else:
            assert np.array_equal(alone[key], v, equal_nan=True), key


@pytest.mark.parametrize("how", ["host", "device"])
def test_scenes_that_are_not_chosen_are_untouched(crowd, how):
    import torch
    chosen = np.zeros(len(ROWS), bool)
    chosen[[1, 3, 8]] = True
    b = _batch()
    try:
        before = _read(b)
        if how == "host":
            b.plan_routes(np.flatnonzero(chosen))
        else:
            b.plan_routes_device(torch.from_numpy(chosen).cuda())
        after = _read(b)
        everything = M._everything(b)
    finally:
        b.close()
    for k in range(len(ROWS)):
        want = crowd[1][k] if chosen[k] else before[k]
        for key, v in want.items():
            if key == "queue":
                assert all(np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) for a, c in zip(after[k][key], v)), (k, key)
            else:
                assert np.array_equal(after[k][key], v, equal_nan=True), (k, key)
    assert len(everything[0]) == len(ROWS)


IDX = (1, 3, 4, 8, 11)                                                # the restart tests' scenes: 2, 300, 5, 5 and 5 rows


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("path", ["host", "device", "auto"])
def test_every_restart_path_plans_from_the_placed_position(path, noise):
    import torch
    b = _batch(IDX)
    try:
        b.plan_routes()
        if noise:
            b.set_restart_noise([5, 6, 7, 8, 9], np.array([1.5, 1.0]), min_gap=0.3, tries=4)
        if path == "auto":
            b.set_episodes(0, max_steps=[1, 1000, 1, 1000, 1])
        b.snapshot()
        snap = _read(b)
        b.run(3)
        chosen = np.array([True, False, True, False, True])
        before = _read(b)
        if path == "host":
            b.restart(np.flatnonzero(chosen))
        elif path == "device":
            b.restart_device(torch.from_numpy(chosen).cuda())
        else:
            b.end_step(auto_restart=True)
            assert np.array_equal(b.episodes()[1], chosen)
        after = _read(b)
    finally:
        b.close()
    # a restarted scene: everything as the snapshot held it, the rows where the restart placed them
    base = [dict(snap[j], loc=after[j]["loc"]) for j in range(len(IDX))]
    seen = _check_all(f"{path}, noise {noise}", SimpleBatchView(True), base, after, IDX, only=chosen)
    assert 1 in seen
    if noise:                                                          # the rows were moved: planned from where they were placed
        assert any(not np.array_equal(after[j]["loc"][:, :2], _world()[0][IDX[j]]["loc"][:, :2]) for j in (0, 2, 4))
    for j in np.flatnonzero(~chosen):                                  # the others: as the ticks left them
        for key in ("wp", "mode", "target", "cursor", "status", "L"):
            assert np.array_equal(after[j][key], before[j][key]), (j, key)


def test_run_after_a_device_plan_equals_a_batch_given_the_route_as_queues():
    """Scene: rows walking along a chain of nodes 3 m apart whose first and fourth edges are crosswalks; with the stock 2 m
    threshold 240 ticks pop several waypoints and put rows into CHECKING_TRAFFIC (4) on the way.  Compared after every tick."""
    import torch
    n, K = 6, 240
    graph = RC.chain(12, spacing=3.0)
    graph["types"] = np.array([2, 1, 1, 2, 1, 1, 2, 1, 1, 1, 1])
    sc, plan, _ = M._scene(n, 2390, 1, borders=2)
    rng = np.random.default_rng(9)
    sc["loc"][:, :2] = f32(np.stack([np.arange(n) * 1.5, 2.5 + np.arange(n) * 0.5], axis=1))
    goals = np.stack([33.0 - np.arange(n) * 2.0, -3.0 + rng.uniform(-1, 1, n)], axis=1)
    gt = np.array([1, 1, 0, 3, 2, 1], np.uint8)
    a = SfmBatch([M._config(0)], [0.05])
    f = SfmBatch([M._config(0)], [0.05])
    try:
        a.upload([sc], device_vehicles=True)
        a.set_modes([plan], despawn_on_arrival=True, arrive_thresholds=2.0, scenes=[sc])
        a.set_routes([graph], [np.maximum(gt, 1)], [goals], mask=[gt != 0], capacity=CAP)
        a.plan_routes_device(torch.ones(1, dtype=torch.uint8, device="cuda"))
        twin = R.plan_scene(R.pack_graph(graph), gt, sc["loc"], goals, CAP)
        assert all(p is None or (p["status"] == 1 and p["L"] >= 4) for p in twin)
        # the fresh batch: the same scene, the twin's routes as ordinary queues, entry 0 as the waypoint
        sc2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
        plan2 = {k: (np.array(v, copy=True) if k != "queues" else [list(q) for q in v]) for k, v in plan.items()}
        for i, p in enumerate(twin):
            if p is None:
                continue
            sc2["waypoint"][i, :2] = p["xy"][0]
            plan2["queues"][i] = [(np.append(p["xy"][j], 0.0), bool(p["cross"][j])) for j in range(1, p["L"])]
            plan2["mode"][i] = 1
            plan2["target_speed"][i] = plan2["initial_speed"][i]
        f.upload([sc2], device_vehicles=True)
        f.set_modes([plan2], despawn_on_arrival=True, arrive_thresholds=2.0, scenes=[sc2])
        c0 = a.modes()[0][2].copy()
        checking = False
        for tick in range(K):
            a.run(1)
            f.run(1)
            (la, va), (lf, vf) = a.state()[0], f.state()[0]
            assert np.array_equal(la, lf) and np.array_equal(va, vf), tick
            (ma, ta, ca), (mf, tf, cf) = a.modes()[0], f.modes()[0]
            assert np.array_equal(ma, mf) and np.array_equal(ta, tf) and np.array_equal(ca - c0, cf), tick
            assert np.array_equal(a.waypoints()[0][0], f.waypoints()[0][0]), tick
            checking = checking or bool((ma[gt != 0] == 4).any())
        popped = (a.modes()[0][2] - c0)[gt != 0]
        assert popped.max() >= 2 and checking, (popped, checking)
    finally:
        a.close()
        f.close()


def test_goals_written_through_the_tensor_are_what_the_next_plan_uses():
    import torch
    b = _batch(IDX)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        g = b.route_goal_tensor()
        st = b.route_status_tensor()
        assert g.shape == (int(b.scene_off[-1]), 2) and st.shape == (int(b.scene_off[-1]),) and st.dtype == torch.int32
        assert int(st.abs().sum()) == 0
        new = torch.stack([torch.linspace(0.0, 40.0, g.shape[0]), torch.linspace(12.0, -3.0, g.shape[0])], dim=1).cuda()
        g.copy_(new)
        before = _read(b)
        b.plan_routes_device(torch.ones(len(IDX), dtype=torch.uint8, device="cuda"))
        after = _read(b)
        status = st.cpu().numpy()
    finally:
        b.close()
    scenes, plans, graphs, gts, _ = _world()
    goals = new.cpu().numpy().astype(np.float64)
    for j, k in enumerate(IDX):
        a, e = int(b.scene_off[j]), int(b.scene_off[j + 1])
        _check_scene(f"tensor goals: scene {k}", before[j], after[j], graphs[k], gts[k], goals[a:e], plans[k]["initial_speed"])
        assert np.array_equal(status[a:e], after[j]["status"])


def test_off_means_off_and_a_3d_batch_ignores_z():
    b = _batch(IDX, z3=True)
    try:
        assert not b.planar
        before = _read(b)
        b.plan_routes()
        after = _read(b)
        _check_all("3-D", b, before, after, IDX)
        zs = [loc[:, 2].copy() for loc, _ in b.state()]
        assert any(np.abs(z).max() > 0.1 for z in zs if len(z))
        b.snapshot()
        b.set_routes(None, None, None)                                 # off: no plan, no buffers, and a restart plans nothing
        assert b.has_snapshot
        for call in (b.plan_routes, b.plan_routes_device, b.routes, b.route_goal_tensor, b.route_status_tensor):
            with pytest.raises(SfmLibraryError, match="routes are off"):
                call()
        rc = b._lib.sfm_batch_plan_routes(b._b, None)
        assert rc == SFM_ERR_STATE and b"routes are off" in b._lib.sfm_batch_last_error(b._b)
        assert not b._lib.sfm_batch_device_ptr(b._b, 13, None) and b"which must be" in b._lib.sfm_batch_last_error(b._b)
        b.run(2)
        m0 = M._everything(b)
        b.restart()
        b.run(2)
        M._assert_same(M._everything(b), m0, "a restart without routes is the plain restart")
    finally:
        b.close()
    # upload and set_modes drop the routes
    b = _batch(IDX)
    try:
        scenes, plans = _world()[:2]
        b.set_modes([plans[k] for k in IDX], scenes=[scenes[k] for k in IDX])
        assert b.route_capacity is None and b._lib.sfm_batch_plan_routes(b._b, None) == SFM_ERR_STATE
    finally:
        b.close()


def test_refusals():
    scenes, plans, graphs, gts, goals = _world()
    pick = lambda v: [v[k] for k in IDX]
    args = (pick(graphs), [np.maximum(g, 1) for g in pick(gts)], pick(goals))
    b = _batch(IDX, routes=False)
    try:
        before = M._everything(b)
        with pytest.raises(SfmLibraryError, match="capacity must be 1 .. 64, got 65"):
            b.set_routes(*args, capacity=65)
        with pytest.raises(SfmLibraryError, match="capacity must be 1 .. 64, got 0"):
            b.set_routes(*args, capacity=0)
        with pytest.raises(ValueError, match="scene 1: nodes: 1025 nodes"):
            b.set_routes([graphs[1], RC.chain(1025)] + pick(graphs)[2:], *args[1:])
        # ... and past the packer: the library's own bound
        node_off = np.array([0, 1025, 1025, 1025, 1025, 1025], np.int32)
        adj_off = np.zeros(1026, np.int32)
        xy = np.zeros(1025, np.float32)
        gt = np.ones(int(b.scene_off[-1]), np.uint8)
        gx = np.zeros(int(b.scene_off[-1]), np.float32)
        rc = b._lib.sfm_batch_set_routes(b._b, iptr(node_off), xy.ctypes.data, xy.ctypes.data, iptr(adj_off), None, None, None,
                                         gt.ctypes.data, gx.ctypes.data, gx.ctypes.data, 16)
        assert rc == SFM_ERR_INVALID and b"scene 0: 1025 nodes" in b._lib.sfm_batch_last_error(b._b)
        with pytest.raises(ValueError, match="scene 0: graph_types"):
            b.set_routes(args[0], [np.full(2, 4)] + args[1][1:], args[2])
        M._assert_same(M._everything(b), before, "a refused set_routes changes nothing")
        assert b.route_capacity is None
        b.set_spawns([None] * len(IDX))
        with pytest.raises(SfmLibraryError, match="spawn schedule"):
            b.set_routes(*args)
        b.set_modes(None)
        with pytest.raises(SfmLibraryError, match="routes need modes"):
            b.set_routes(*args)
    finally:
        b.close()


def test_the_example_loop_plans_on_the_device():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("batch_routed_loop", os.path.join(root, "examples", "batch_routed_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    episodes, routes, per_status = mod.run(B=8, steps=12, repeat=2, max_age=5, quiet=True)
    assert episodes == 8 * 2 and routes > 0 and per_status.sum() == 8 * mod.N_B and per_status[0] == 0 and per_status[4:].sum() == 0
