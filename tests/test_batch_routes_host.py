"""Host tests of the routes over walk graphs (carla_social_force_model_amd.route: pack_graphs, plan_row, plan_scene,
usable_nodes -- the NumPy twins of sfm_batch_plan_routes_kernel): against routes of the reference's own planner
(tests/golden/routes/*.npz, written by tests/golden/make_golden_routes.py from the cases of tests/_route_cases.py), on designed
cases that meet every branch of the rule, and the packer's refusals.  No GPU.

A case of the fixture may be left out of the comparison only when a float64 decision of the reference lies inside the rounding
bound derived in tests/_route_cases.py: the gap between the best and the second-best simple path, the two trim comparisons and
the two nearest-node choices.  The test keeps itself honest: the reference answers at least 80 % of the cases and at most 5 % of
the answered ones are left out."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _golden_io as gio
import _route_cases as RC
from carla_social_force_model_amd import _lib, batch, route as R

ROUTES_DIR = os.path.join(gio.GOLDEN_DIR, "routes")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    z = np.load(os.path.join(ROUTES_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _nearest_margin_ok(graph, ok, p, chosen):
    """Is the float64 choice of the nearest usable node outside the fp32 rounding bound?"""
    nodes = np.asarray(graph["nodes"], np.float64)
    best = RC.d2_64(nodes[chosen], p)
    for v in np.flatnonzero(ok):
        if v != chosen and RC.d2_64(nodes[v], p) - best <= RC.d2_bound(nodes[v], p) + RC.d2_bound(nodes[chosen], p):
            return False
    return True


def _trim_margin_ok(a, b, c):
    """the decision d(a, b) > d(c, b), taken in float64, outside the fp32 rounding bound"""
    return abs(RC.d2_64(a, b) - RC.d2_64(c, b)) > RC.d2_bound(a, b) + RC.d2_bound(c, b)


def _compare_set(name, tie_ok=False):
    """-> (queries, answered, left out, compared)"""
    fx = _load(name)
    cases = RC.reference_sets()[name]
    assert str(fx["digest"]) == RC.digest(cases), "the fixture was made from other inputs: run tests/golden/make_golden_routes.py"
    q = answered = left_out = compared = 0
    for graph, queries in cases:
        g = R.pack_graph(graph)
        nodes = np.asarray(graph["nodes"], np.float64)
        for o, d, gt in queries:
            k = q
            q += 1
            p = R.plan_row(g, gt, o, d, capacity=R.MAX_CAPACITY)
            ok = R.usable_nodes(g, gt)
            if fx["raised"][k]:
                # NodeNotFound: the node nearest in the whole graph is not in the sub-graph -- the documented departure (the rule
                # takes the nearest usable node instead); NetworkXNoPath: the rule reports status 2
                if fx["raised"][k] == 1 and ok[fx["s"][k]] and ok[fx["t"][k]]:
                    assert p["status"] == R.STATUS_NO_PATH, (name, k)
                continue
            answered += 1
            s, t = int(fx["s"][k]), int(fx["t"][k])
            ref_path = fx["path"][fx["path_off"][k]:fx["path_off"][k + 1]].tolist()
            a, b = fx["route_off"][k], fx["route_off"][k + 1]
            ref_xy, ref_cross = fx["route_xy"][a:b], fx["route_cross"][a:b]
            # the float64 decisions that fp32 may take differently
            skip = not _nearest_margin_ok(graph, ok, o, s) or not _nearest_margin_ok(graph, ok, d, t)
            if not skip and np.isfinite(fx["second"][k]):
                hops = max(int(fx["hops"][k]), int(fx["hops2"][k]))
                tie = fx["second"][k] - fx["best"][k] <= RC.path_bound(hops, fx["second"][k])
                if tie and tie_ok:                                    # an exact tie: any of the reference's equal-cost routes
                    assert p["status"] == R.STATUS_PLANNED and (p["s"], p["t"]) == (s, t), (name, k)
                    cost64 = sum(np.linalg.norm(nodes[u] - nodes[v]) for u, v in zip(p["nodes"][:-1], p["nodes"][1:]))
                    assert abs(cost64 - fx["best"][k]) <= RC.path_bound(hops, fx["best"][k]), (name, k)
                    compared += 1
                    continue
                skip = tie
            full = p["nodes"]
            if not skip and p["status"] == R.STATUS_PLANNED and len(full) > 1:
                skip = (not _trim_margin_ok(nodes[full[0]], nodes[full[1]], o) or
                        not _trim_margin_ok(nodes[full[-1]], nodes[full[-2]], d))
            if skip:
                left_out += 1
                continue
            compared += 1
            assert p["status"] == R.STATUS_PLANNED and (p["s"], p["t"]) == (s, t), (name, k, p["status"], p["s"], p["t"], s, t)
            first = int(len(full) > 1 and R.d2(g["xy"][full[0]], g["xy"][full[1]]) > R.d2(np.float32(o[:2]), g["xy"][full[1]]))
            last = int(len(full) > 1 and R.d2(g["xy"][full[-1]], g["xy"][full[-2]]) > R.d2(np.float32(d[:2]), g["xy"][full[-2]]))
            assert full[first:len(full) - last] == ref_path, (name, k, full, ref_path)           # the node sequence after trimming
            assert p["L"] == len(ref_cross) and np.array_equal(p["cross"], ref_cross), (name, k)
            assert np.array_equal(p["xy"], ref_xy[:, :2].astype(np.float32)), (name, k)          # the waypoints, rounded once
    return q, answered, left_out, compared


def test_twin_equals_the_reference_on_random_street_grids():
    q, answered, left_out, compared = _compare_set("random")
    print(f"random: {q} queries, {answered} answered by the reference, {left_out} left out, {compared} compared")
    assert q == 800 and answered >= 0.8 * q and left_out <= 0.05 * answered and compared == answered - left_out


def test_twin_equals_the_reference_on_designed_cases():
    q, answered, left_out, compared = _compare_set("designed", tie_ok=True)
    print(f"designed: {q} queries, {answered} answered by the reference, {left_out} left out, {compared} compared")
    assert answered >= 0.8 * q and left_out <= 0.05 * answered and compared == answered - left_out


def test_committed_digests_are_what_the_generator_builds_today(tmp_path):
    gen = os.path.join(gio.GOLDEN_DIR, "make_golden_routes.py")
    subprocess.check_call([sys.executable, gen, "--inputs-only", "--out", str(tmp_path)], stdout=subprocess.DEVNULL)
    names = sorted(f[:-4] for f in os.listdir(ROUTES_DIR) if f.endswith(".npz"))
    assert names == ["designed", "random"]
    for name in names:
        new = np.load(tmp_path / (name + ".npz"), allow_pickle=False)
        assert str(new["digest"]) == str(_load(name)["digest"]), name
        assert os.path.getsize(os.path.join(ROUTES_DIR, name + ".npz")) < 64 * 1024, name
    assert str(_load("random")["networkx"]) == "3.4.2"


# ---- designed cases, branch by branch ------------------------------------------------------------------------------------------
def _z(x, y):
    return np.array([x, y, 0.0])


def test_exact_ties_take_the_lowest_neighbour():
    g = R.pack_graph(RC.integer_grid(5))
    p = R.plan_row(g, 1, _z(0.4, 0.3), _z(12.3, 11.6))
    assert (p["s"], p["t"], p["status"]) == (0, 24, 1) and float(p["cost"]) == 24.0
    # from every node next is the lower of the two neighbours that are nearer to t: +x (v + 1) before +y (v + 5)
    assert p["nodes"] == [0, 1, 2, 3, 4, 9, 14, 19, 24]
    q = R.plan_row(g, 3, _z(11.8, 0.2), _z(0.3, 12.4))
    assert q["nodes"] == [4, 3, 2, 1, 0, 5, 10, 15, 20] and float(q["cost"]) == 24.0


def test_trims_each_alone_both_and_neither():
    g = R.pack_graph(RC.chain(6, spacing=5.0))
    both = R.plan_row(g, 1, _z(2.0, 0.5), _z(23.0, -0.5))
    assert both["nodes"] == [0, 1, 2, 3, 4, 5] and both["L"] == 5
    assert np.array_equal(both["xy"][:, 0], np.float32([5, 10, 15, 20, 23])) and not both["cross"].any()
    first = R.plan_row(g, 1, _z(2.0, 0.5), _z(26.0, 0.3))
    assert first["L"] == 6 and first["xy"][0, 0] == 5 and first["xy"][-2, 0] == 25
    last = R.plan_row(g, 1, _z(-1.0, 0.2), _z(23.0, 0.4))
    assert last["L"] == 6 and last["xy"][0, 0] == 0 and last["xy"][-2, 0] == 20
    neither = R.plan_row(g, 1, _z(-1.0, 0.2), _z(26.0, 0.3))
    assert neither["L"] == 7 and neither["xy"][0, 0] == 0 and neither["xy"][-2, 0] == 25
    two = R.plan_row(g, 1, _z(1.0, 0.1), _z(4.0, 0.1))               # a two-node route with both nodes trimmed: the goal alone
    assert two["nodes"] == [0, 1] and two["status"] == 1 and two["L"] == 1 and np.array_equal(two["xy"], np.float32([[4.0, 0.1]]))
    same = R.plan_row(g, 2, _z(11.0, 0.3), _z(9.0, -0.3))            # s == t
    assert same["nodes"] == [2] and same["status"] == 1 and same["L"] == 1 and float(same["cost"]) == 0.0


def test_three_graph_types_three_routes_and_a_factor_that_flips_one():
    g = R.pack_graph(RC.three_ways(2.0))
    o, d = _z(-0.5, -0.5), _z(24.5, -0.5)
    no, junction, anywhere = (R.plan_row(g, t, o, d) for t in (1, 2, 3))
    assert no["nodes"] == [0, 2, 4, 5, 3, 1] and junction["nodes"] == [0, 2, 3, 1] and anywhere["nodes"] == [0, 6, 7, 1]
    assert no["cross"].tolist() == [0, 0, 0, 1, 0, 0, 0] and junction["cross"].tolist() == [0, 0, 1, 0, 0]
    assert anywhere["cross"].tolist() == [0, 0, 1, 0, 0]               # (sidewalk to road is no crossing; the jaywalk is)
    assert float(junction["cost"]) == 30 + 2 * 24 + 30 and float(anywhere["cost"]) == 2 + 2 * 20 + 2
    dear = R.pack_graph(RC.three_ways(4.0))                           # jaywalking four times as dear: graph type 3 takes the junction
    assert R.plan_row(dear, 3, o, d)["nodes"] == [0, 6, 7, 1] and float(R.plan_row(dear, 3, o, d)["cost"]) == 84.0
    dearer = R.pack_graph(RC.three_ways(8.0))
    assert R.plan_row(dearer, 3, o, d)["nodes"] == [0, 2, 4, 5, 3, 1]   # ... and eight times: the crosswalk (144 < 164, 252)
    assert np.array_equal(R.usable_nodes(g, 1), [1, 1, 1, 1, 1, 1, 0, 0]) and R.usable_nodes(g, 3).all()


def test_status_values():
    g = R.pack_graph(RC.two_components())
    assert R.plan_row(g, 1, _z(1, 1), _z(104, 5))["status"] == R.STATUS_NO_PATH                      # t not reachable from s
    lone = R.pack_graph({"nodes": [[0, 0], [5, 0]], "edges": [[0, 1]], "types": [3]})
    p = R.plan_row(lone, 1, _z(1, 1), _z(4, 0))                                                       # no usable node
    assert p["status"] == R.STATUS_NO_PATH and (p["s"], p["t"], p["L"]) == (-1, -1, 1) and np.array_equal(p["xy"], np.float32([[4, 0]]))
    assert R.plan_row(R.pack_graph({"nodes": np.zeros((0, 2)), "edges": [], "types": []}), 1, _z(1, 1), _z(4, 0))["status"] == 2
    ch = R.pack_graph(RC.chain(12))
    fits = R.plan_row(ch, 1, _z(-1, 0), _z(34, 0), capacity=12)
    short = R.plan_row(ch, 1, _z(-1, 0), _z(34, 0), capacity=11)                                      # one short
    assert (fits["status"], fits["L"]) == (1, 13) and (short["status"], short["L"]) == (R.STATUS_TOO_LONG, 13)
    assert np.array_equal(short["xy"], np.float32([[34, 0]]))
    for bad in (np.nan, np.inf, -np.inf, 1e39):
        assert R.plan_row(ch, 1, _z(-1, 0), _z(bad, 0))["status"] == R.STATUS_BAD_GOAL
    rows = R.plan_scene(ch, [1, 0, 2, 1], [[0, 0], [1, 1], [3e15, 0], [2, 0]], [[9, 0]] * 4, modes=[1, 1, 1, 255])
    assert [None if r is None else r["status"] for r in rows] == [1, None, R.STATUS_NOT_LIVE, R.STATUS_NOT_LIVE]
    assert R.queue_slots(fits, 16)[0] == 4 and R.queue_slots(short, 16)[0] == 16


@pytest.mark.parametrize("lengths", ["zero", "absorbed"])
def test_next_has_no_cycle_with_zero_length_edges_and_absorbed_adds(lengths):
    rng = np.random.default_rng(77)
    for trial in range(20):
        graph = RC.random_graph(40, 7700 + trial)
        E = len(graph["edges"])
        if lengths == "zero":
            graph["lengths"] = np.where(rng.random(E) < 0.6, 0.0, rng.integers(1, 4, E).astype(float))
        else:
            graph["lengths"] = np.where(rng.random(E) < 0.5, 1e-3, 1e8)         # fl(1e8 + 1e-3) == 1e8: an add that changes nothing
        g = R.pack_graph(graph)
        for t in range(0, 40, 7):
            D, nxt, rounds = R.distance_field(g, 3, t)
            assert rounds <= 40
            for v in range(40):                                       # every walk ends in t within V - 1 hops
                u, hops = v, 0
                while u != t and nxt[u] >= 0 and hops < 40:
                    w = g["nbr"][nxt[u]]
                    assert D[w] <= D[u]
                    u, hops = int(w), hops + 1
                assert hops < 40 and (u == t or not np.isfinite(D[v]))
            # the field is the fixed point: no edge improves it
            src = np.repeat(np.arange(40), np.diff(g["off"]))
            assert not ((D[g["nbr"]] + g["w"]).astype(np.float32) < D[src]).any()


def test_result_is_independent_of_the_order_of_the_edges():
    rng = np.random.default_rng(5)
    graph = RC.street_grid(5, 4, 99)
    base = R.pack_graph(graph)
    perm = rng.permutation(len(graph["edges"]))
    flip = rng.random(len(perm)) < 0.5
    e = graph["edges"][perm]
    e = np.where(flip[:, None], e[:, ::-1], e)
    other = R.pack_graph({**graph, "edges": e, "types": graph["types"][perm]})
    for k in base:
        assert np.array_equal(base[k], other[k]), k
    # a duplicate edge overrides the one before it, as nx.Graph.add_edge does
    dup = R.pack_graph({"nodes": [[0, 0], [3, 0]], "edges": [[0, 1], [1, 0]], "types": [1, 3], "lengths": [3.0, 4.0]})
    assert dup["typ"].tolist() == [3, 3] and dup["w"].tolist() == [8.0, 8.0] and dup["nbr"].tolist() == [1, 0]


def test_weights_are_formed_in_fp32():
    g = R.pack_graph({"nodes": [[0, 0], [0.1, 0.2], [7, 7]], "edges": [[0, 1], [1, 2], [0, 2]], "types": [3, 1, 4],
                      "jaywalking_weight_factor": 1.1})
    L = np.float32(np.sqrt(np.float64(0.1) ** 2 + np.float64(0.2) ** 2))
    assert g["w"][0] == np.float32(L * np.float32(1.1)) and g["w"][1] == np.float32(np.float32(np.sqrt(98.0)) * np.float32(1.1))
    assert g["w"][0] == g["w"][2] and g["w"][1] == g["w"][4] and g["w"][3] == g["w"][5] == np.float32(np.sqrt(6.9 ** 2 + 6.8 ** 2)) and g["off"].tolist() == [0, 2, 4, 6] and g["nbr"].tolist() == [1, 2, 0, 2, 0, 1]


def test_packer_refusals_name_scene_and_key():
    ok = {"nodes": [[0, 0], [3, 0], [6, 0]], "edges": [[0, 1], [1, 2]], "types": [1, 2]}
    for change, words in (({"edges": [[0, 3], [1, 2]]}, ("scene 1", "edges[0]", "out of range")),
                          ({"edges": [[0, 1], [2, 2]]}, ("scene 1", "edges[1]", "self loop")),
                          ({"types": [1, -1]}, ("scene 1", "types[1]", "VOID")),
                          ({"types": [1, 6]}, ("scene 1", "types[1]")),
                          ({"types": [1]}, ("scene 1", "types")),
                          ({"lengths": [1.0, -1.0]}, ("scene 1", "lengths[1]")),
                          ({"lengths": [np.nan, 1.0]}, ("scene 1", "lengths[0]")),
                          ({"lengths": [1.0]}, ("scene 1", "lengths")),
                          ({"nodes": [[0, 0], [np.inf, 0], [6, 0]]}, ("scene 1", "nodes")),
                          ({"nodes": [0, 1, 2]}, ("scene 1", "nodes")),
                          ({"jaywalking_weight_factor": -1}, ("scene 1", "jaywalking_weight_factor")),
                          ({"weights": [1, 2]}, ("scene 1", "weights"))):
        with pytest.raises(ValueError) as ei:
            R.pack_graphs([None, {**ok, **change}])
        assert all(w in str(ei.value) for w in words), (change, str(ei.value))
    with pytest.raises(ValueError, match="scene 0: nodes: 1025 nodes"):
        R.pack_graphs([RC.chain(1025)])
    pg = R.pack_graphs([None, ok, RC.chain(4), None])
    assert pg["node_off"].tolist() == [0, 0, 3, 7, 7] and pg["adj_off"].tolist() == [0, 1, 3, 4, 5, 7, 9, 10]
    assert pg["adj_node"].tolist() == [1, 0, 2, 1, 1, 0, 2, 1, 3, 2] and pg["scenes"][0] is None
    with pytest.raises(ValueError, match="graph type"):
        R.kept([1], 4)


def test_header_bindings_and_constants_agree():
    with open(os.path.join(ROOT, "include", "sfm_hip.h")) as f:
        src = f.read()
    for name in ("sfm_batch_set_routes", "sfm_batch_plan_routes", "sfm_batch_plan_routes_device", "sfm_batch_download_routes"):
        assert re.search(r"\bint " + name + r"\(SfmBatch\* b", src) and name in _lib.SYMBOLS and name in _lib.UNBUMPED
    for name, val in (("SFM_BATCH_PTR_ROUTE_GOALS", batch.PTR_ROUTE_GOALS), ("SFM_BATCH_PTR_ROUTE_STATUS", batch.PTR_ROUTE_STATUS),
                      ("SFM_BATCH_MAX_ROUTE_NODES", R.MAX_NODES), ("SFM_BATCH_MAX_ROUTE_CAPACITY", R.MAX_CAPACITY)):
        assert re.search(r"#define " + name + " " + str(val) + r"\b", src), name
    assert re.search(r"#define SFM_ABI_VERSION 17\b", src) and _lib.ABI_VERSION == 17
    with open(os.path.join(ROOT, "carla-social-force-model_amd", "csrc", "sfm_device.h")) as f:
        dev = f.read()
    assert "ROUTE_MAX_NODES = 1024" in dev and "ROUTE_MAX_CAPACITY = 64" in dev


def test_per_row_arguments():
    so = np.array([0, 2, 2, 5], np.int32)
    gt, gx, gy = batch.pack_route_rows([np.array([1, 3], np.uint8), 2, 3], [[[1, 2], [3, 4]], None, [5.0, 6.0, 7.0]],
                                       [None, None, [True, False, True]], so)
    assert gt.tolist() == [1, 3, 3, 0, 3] and gx.tolist() == [1, 3, 5, 5, 5] and gy.tolist() == [2, 4, 6, 6, 6]
    assert batch.pack_route_rows(2, np.zeros((5, 2)), None, so)[0].tolist() == [2] * 5
    for bad, words in ((([1, 2], np.zeros((5, 2)), None), "graph_types: 2 entries"),
                       (([1, 2, [1, 2, 4]], np.zeros((5, 2)), None), "scene 2: graph_types"),
                       (([1, 2, 0], np.zeros((5, 2)), None), "scene 2: graph_types"),
                       ((1, np.zeros((5, 2)), [None, None, [True]]), "scene 2: mask"),
                       ((1, np.zeros((4, 2)), None), "goals")):
        with pytest.raises(ValueError, match=words):
            batch.pack_route_rows(*bad, so)


def test_the_example_imports_without_a_gpu():
    import importlib.util
    spec = importlib.util.spec_from_file_location("batch_routed_loop", os.path.join(ROOT, "examples", "batch_routed_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    scenes, plans, graphs = mod.make_world(3)
    assert len(scenes) == len(plans) == len(graphs) == 3 and 2 * (mod.SIDE - 1) + 1 <= mod.CAPACITY
    g = R.pack_graph(graphs[0])
    assert g["xy"].shape == (mod.SIDE ** 2, 2) and all(len(q) == 0 for q in plans[0]["queues"])
    src = open(os.path.join(ROOT, "examples", "batch_routed_loop.py")).read()
    loop = src[src.index("for step in range(steps):"):src.index("per_status =")]
    assert ".cpu()" not in loop and "synchronize" not in loop and "b.routes()" not in loop      # nothing on the host inside the loop
