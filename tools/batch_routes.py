"""Routes planned on the device (sfm_batch_set_routes): B = 1024 scenes of 64, all five forces, 4 moving device-side vehicles per
scene, a jittered 10 x 10 street grid (100 nodes, 180 edges of mixed types) per scene, goals drawn from the graph's nodes.
  --part run     `rounds` rounds of `calls` restart_device() calls and of one run(ticks) call with NO routes set -- what a batch
                 that never sets routes launches; run once per library build (SFM_LIB_PATH names another build) and alternated by
                 tools/batch_routes.sh: this build against its parent
  --part plan    alternated in `rounds` rounds (us per call, medians at the end): plan_routes_device() over every scene with one
                 routed row (the agent) per scene; the same with every row routed; and the host path a caller has without it for
                 one agent per scene: download the state, the reference's search (nx.astar_path on the scene's sub-graph, with
                 the trims), and set_modes with the new queues
  --part trace   `calls` plan_routes_device() calls with one routed row per scene, then with every row -- for rocprofv3
                 --kernel-trace --stats: the plan kernel's own duration
Times are host wall clock around the calls, closed by a device synchronisation."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from carla_social_force_model_amd import scenarios  # noqa: E402
from carla_social_force_model_amd.batch import SfmBatch  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402

POOL = 32
DT = 0.05
N_B = 64
CAP = 32
SIDE = 10


def _sync():
    import torch
    torch.cuda.synchronize()


def _timed(fn):
    _sync()
    t0 = time.perf_counter()
    fn()
    _sync()
    return time.perf_counter() - t0


def _scenes(B):
    pool = []
    for k in range(POOL):
        sc = vars(scenarios.make_scenario(N_B, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0)))
        plan, _ = scenarios.make_mode_plan(sc, 7100 + k, queue_len=1)
        pool.append((sc, plan))
    return [pool[k % POOL][0] for k in range(B)], [pool[k % POOL][1] for k in range(B)]


def _street_grid(seed, spacing=4.0, jitter=0.8):
    """a jittered SIDE x SIDE street grid, mostly sidewalks, with crosswalks and the three jaywalking types mixed in"""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.arange(SIDE) * spacing, np.arange(SIDE) * spacing)
    nodes = np.stack([xs.ravel(), ys.ravel()], axis=1) + rng.uniform(-jitter, jitter, (SIDE * SIDE, 2))
    v = np.arange(SIDE * SIDE).reshape(SIDE, SIDE)
    edges = np.concatenate([np.stack([v[:, :-1].ravel(), v[:, 1:].ravel()], axis=1), np.stack([v[:-1].ravel(), v[1:].ravel()], axis=1)])
    return {"nodes": nodes, "edges": edges, "types": rng.choice([1, 2, 3, 4, 5], len(edges), p=[0.7, 0.12, 0.06, 0.08, 0.04])}


def _graphs(B):
    pool = [_street_grid(7200 + k) for k in range(POOL)]
    return [pool[k % POOL] for k in range(B)]


def _host_plan(b, graphs, nxg, goals, scenes, plans):
    """What a caller does without the feature, for the agent (row 0) of every scene: the state to the host, the reference's search
    on the JAYWALKING_AT_JUNCTION sub-graph, the queues up again with set_modes."""
    import networkx as nx
    state = b.state()
    new = []
    for k, (g, G) in enumerate(zip(graphs, nxg)):
        nodes = g["nodes"]
        o, d = state[k][0][0, :2], goals[k][0, :2]
        live = np.fromiter(G.nodes, int)
        s = int(live[np.argmin(((nodes[live] - o) ** 2).sum(1))])
        t = int(live[np.argmin(((nodes[live] - d) ** 2).sum(1))])
        try:
            path = nx.astar_path(G, s, t, heuristic=lambda a, c: float(np.linalg.norm(nodes[a] - nodes[c])), weight="length")
        except nx.NetworkXNoPath:
            path = []
        if len(path) > 1:
            first = np.linalg.norm(nodes[path[0]] - nodes[path[1]]) > np.linalg.norm(o - nodes[path[1]])
            last = np.linalg.norm(nodes[path[-1]] - nodes[path[-2]]) > np.linalg.norm(d - nodes[path[-2]])
            path = path[int(first):len(path) - int(last)]
        q = [(np.append(nodes[v], 0.0), G.edges[u, v]["type"] in (2, 3, 4)) for u, v in zip(path[:-1], path[1:])] if len(path) > 1 else []
        q.append((np.append(d, 0.0), False))
        plan = dict(plans[k])
        plan["queues"] = [q] + list(plans[k]["queues"][1:])
        new.append(plan)
    b.set_modes(new, scenes=scenes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("run", "plan", "trace"), default="plan")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    ap.add_argument("--scenes", type=int, default=1024)
    args = ap.parse_args()
    import torch
    B = args.scenes
    what = f"B = {B} scenes of {N_B}, all five forces, 4 moving device-side vehicles per scene"
    scenes, plans = _scenes(B)
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        b.upload(scenes, device_vehicles=True)
        b.set_modes(plans, scenes=scenes)
        if args.part == "run":
            b.run(3)
            b.snapshot()
            mask = np.zeros(B, bool)
            mask[::8] = True
            d_mask = torch.from_numpy(mask).cuda()

            def restarts():
                for _ in range(args.calls):
                    b.restart_device(d_mask)

            print(f"# {args.label}: no routes set, {what}, every eighth scene restarted "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            restarts()
            b.run(3)
            for r in range(args.rounds):
                t = _timed(restarts) / args.calls
                u = _timed(lambda: b.run(args.ticks)) / args.ticks
                print(f"{args.label:<8} {B:>6} {N_B:>5} {r:>5} {t * 1e6:>14.1f} {u * 1e6:>10.1f}", flush=True)
            return
        graphs = _graphs(B)
        rng = np.random.default_rng(23)
        goals = [g["nodes"][rng.integers(0, len(g["nodes"]), N_B)] + rng.uniform(-1.0, 1.0, (N_B, 2)) for g in graphs]
        one = [np.arange(N_B) == 0] * B
        every = torch.ones(B, dtype=torch.uint8, device="cuda")
        from carla_social_force_model_amd import route as R
        packed = R.pack_graphs(graphs)

        def plans_(calls=args.calls):
            for _ in range(calls):
                b.plan_routes_device(every)

        def routed(mask):
            b.set_routes(packed, 2, goals, mask=mask, capacity=CAP)

        if args.part == "plan":
            import networkx as nx
            nxg = []
            for g in graphs[:POOL]:
                G = nx.Graph()
                d = g["nodes"][g["edges"][:, 0]] - g["nodes"][g["edges"][:, 1]]
                for (u, v), t, ln in zip(g["edges"], g["types"], np.sqrt((d * d).sum(1))):
                    if t not in (3, 5):
                        G.add_edge(int(u), int(v), length=float(ln) * (2.0 if t == 4 else 1.0), type=int(t))
                nxg.append(G)
            nxg = [nxg[k % POOL] for k in range(B)]
            print(f"# plan: {what}; a {SIDE} x {SIDE} street grid per scene, capacity {CAP}, graph type 2; us per call")
            print(f"{'form':<72} {'round':>5} {'us/call':>12}")
            names = ("plan_routes_device(), one routed row per scene", "plan_routes_device(), every row routed",
                     "the host path, one row per scene: download, nx.astar_path, set_modes")
            got = {n: [] for n in names}
            for r in range(args.rounds):
                routed(one)
                plans_(3)
                got[names[0]].append(_timed(plans_) / args.calls)
                st1 = np.bincount(np.concatenate([q["status"] for q in b.routes()]), minlength=6)
                routed(None)
                plans_(3)
                got[names[1]].append(_timed(plans_) / args.calls)
                st2 = np.bincount(np.concatenate([q["status"] for q in b.routes()]), minlength=6)
                got[names[2]].append(_timed(lambda: _host_plan(b, graphs, nxg, goals, scenes, plans)))
                for n in names:
                    print(f"{n:<72} {r:>5} {got[n][-1] * 1e6:>12.1f}", flush=True)
            print(f"# rows by status 0..5, one routed row per scene: {st1.tolist()}; every row: {st2.tolist()}")
            print("# medians (us), and each over the first")
            ref = statistics.median(got[names[0]])
            for n in names:
                m = statistics.median(got[n])
                print(f"{n:<72} {'med':>5} {m * 1e6:>12.1f} {m / ref:>9.2f}x")
        else:
            routed(one)
            t1 = _timed(plans_) / args.calls
            routed(None)
            t2 = _timed(plans_) / args.calls
            print(f"# trace: {args.calls} plan_routes_device() calls with one routed row per scene ({t1 * 1e6:.1f} us per call), then "
                  f"{args.calls} with every row routed ({t2 * 1e6:.1f} us per call), {what} (wall clock, under the tracer)")
    finally:
        b.close()


if __name__ == "__main__":
    main()
