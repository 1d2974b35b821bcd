#!/usr/bin/env python3
"""Golden routes from the REFERENCE's own planner: path_planner.PedPathPlanner imported unmodified, with the installed networkx
(the fixture records its version).  Build-container only.

The planner builds its graph from a CARLA map; that part is not what the batch restates.  Here the planner is made with
``PedPathPlanner.__new__`` and given an empty ``nx.Graph``, ``id_map``, ``road_id_to_edge`` and a map object whose
``get_waypoint`` returns the location itself with one fixed (road, section, lane); the hand-built graphs of tests/_route_cases.py
are then fed, edge by edge as waypoint pairs, through the reference's own ``_generate_edge_dicts``,
``_add_topology_edges_to_graph`` and ``_extract_subgraphs``.  ``carla`` is the stand-in of tests/golden/_standins_routes
(``Location.distance`` and the ``LaneType`` names).  Recorded per query: ``_path_search`` translated to the caller's node indices
through ``id_map``, ``generate_route`` (waypoints and crossing flags), and which queries raised (NetworkXNoPath, NodeNotFound).
Also recorded, for the float64 decisions the fp32 rule may legitimately take differently: cost and hops of the best and the
second-best simple path (``nx.shortest_simple_paths`` on the reference's own sub-graph), so the test needs no networkx.

With one (road, section, lane) for every edge, ``_find_closest_node_id`` walks every edge of the whole graph: it returns the node
nearest to the location, whether or not the sub-graph of the query's graph type holds it (if not, ``nx.astar_path`` raises).

Inputs come from tests/_route_cases.py and are not stored; each fixture holds the SHA-256 of its inputs.  ``--inputs-only``
writes the digests alone (no reference code runs): the drift guard of tests/test_batch_routes_host.py.  Files are written with
fixed zip time stamps, so a re-run reproduces them byte for byte."""
import argparse
import io
import itertools
import os
import sys
import zipfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import _route_cases as RC                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--inputs-only", action="store_true")
ap.add_argument("--out", default=os.path.join(HERE, "routes"))
args = ap.parse_args()


def save(name, **arrays):
    """np.savez_compressed with fixed time stamps."""
    os.makedirs(args.out, exist_ok=True)
    with zipfile.ZipFile(os.path.join(args.out, name + ".npz"), "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


sets = RC.reference_sets()
digests = {k: RC.digest(v) for k, v in sets.items()}

if args.inputs_only:
    for name, d in digests.items():
        save(name, digest=np.array(d))
    sys.exit(0)

REF = os.environ.get("SFM_REFERENCE", "/root/reference")
if not os.path.isdir(REF):
    print("reference checkout not present -- nothing to do")
    sys.exit(0)

sys.path.insert(1, os.path.join(HERE, "_standins_routes"))
sys.path.insert(0, REF)
import carla                                              # noqa: E402  (the routes stand-in)
import networkx as nx                                     # noqa: E402
from path_planner import EdgeType, GraphType, PedPathPlanner     # noqa: E402  (reference)

ROAD, SECTION, LANE = 1, 0, 1
RAISED = {"none": 0, "NetworkXNoPath": 1, "NodeNotFound": 2}


def waypoint(p):
    loc = carla.Location(float(p[0]), float(p[1]), float(p[2]) if len(p) > 2 else 0.0)
    return SimpleNamespace(transform=SimpleNamespace(location=loc), road_id=ROAD, section_id=SECTION, lane_id=LANE,
                           lane_type=carla.LaneType.Sidewalk)


class Map:
    def get_waypoint(self, location, lane_type=None):
        return waypoint((location.x, location.y, location.z))


def planner_for(graph):
    pl = PedPathPlanner.__new__(PedPathPlanner)
    pl.jaywalking_weight_factor = float(graph.get("jaywalking_weight_factor", 2.0))
    pl.carla_map = Map()
    pl.graph = nx.Graph()
    pl.id_map = {}
    pl.road_id_to_edge = {}
    wps = [waypoint(p) for p in graph["nodes"]]
    for (a, b), t in zip(graph["edges"], graph["types"]):
        pl._add_topology_edges_to_graph(pl._generate_edge_dicts([wps[int(a)], wps[int(b)]], EdgeType(int(t))))
    pl._extract_subgraphs()
    # the reference's node ids (order of first appearance) -> the caller's indices, through the rounded coordinates
    mine = {tuple(np.round([p[0], p[1], p[2] if len(p) > 2 else 0.0], 0)): k for k, p in enumerate(graph["nodes"])}
    assert len(mine) == len(graph["nodes"]), "two nodes round to the same integers"
    back = {i: mine[xyz] for xyz, i in pl.id_map.items()}
    return pl, back


for name, cases in sets.items():
    rows = {k: [] for k in ("raised", "path_off", "path", "route_off", "route_xy", "route_cross", "best", "second", "hops",
                            "hops2", "s", "t")}
    rows["path_off"].append(0)
    rows["route_off"].append(0)
    for graph, queries in cases:
        pl, back = planner_for(graph)
        for o, d, g in queries:
            sub = pl.graph_dict[GraphType(int(g))]
            origin, dest = carla.Location(*map(float, o)), carla.Location(*map(float, d))
            s, t = pl._find_closest_node_id(origin), pl._find_closest_node_id(dest)
            raised, path, route = "none", [], []
            try:
                path = pl._path_search(sub, origin, dest)
                route = pl.generate_route(np.asarray(o, float), np.asarray(d, float), GraphType(int(g)))
            except nx.NetworkXNoPath:
                raised = "NetworkXNoPath"
            except nx.NodeNotFound:
                raised = "NodeNotFound"
            best = second = np.inf
            hops = hops2 = 0
            if raised == "none" and s != t:
                two = list(itertools.islice(nx.shortest_simple_paths(sub, s, t, weight="length"), 2))
                cost = lambda p: float(sum(sub.edges[(a, b)]["length"] for a, b in zip(p[:-1], p[1:])))
                best, hops = cost(two[0]), len(two[0]) - 1
                if len(two) > 1:
                    second, hops2 = cost(two[1]), len(two[1]) - 1
            elif raised == "none":
                best = 0.0
            rows["raised"].append(RAISED[raised])
            rows["s"].append(-1 if s is None else back[s])
            rows["t"].append(-1 if t is None else back[t])
            rows["path"] += [back[v] for v in path]
            rows["path_off"].append(len(rows["path"]))
            rows["route_xy"] += [[float(w[0]), float(w[1]), float(w[2])] for w, _ in route]
            rows["route_cross"] += [int(bool(c)) for _, c in route]
            rows["route_off"].append(len(rows["route_cross"]))
            rows["best"].append(best)
            rows["second"].append(second)
            rows["hops"].append(hops)
            rows["hops2"].append(hops2)
    raised = np.asarray(rows["raised"], np.uint8)
    save(name, raised=raised, s=np.asarray(rows["s"], np.int32), t=np.asarray(rows["t"], np.int32),
         path_off=np.asarray(rows["path_off"], np.int32), path=np.asarray(rows["path"], np.int32),
         route_off=np.asarray(rows["route_off"], np.int32), route_xy=np.asarray(rows["route_xy"], np.float64).reshape(-1, 3),
         route_cross=np.asarray(rows["route_cross"], np.uint8), best=np.asarray(rows["best"], np.float64),
         second=np.asarray(rows["second"], np.float64), hops=np.asarray(rows["hops"], np.int32),
         hops2=np.asarray(rows["hops2"], np.int32), digest=np.array(digests[name]), networkx=np.array(nx.__version__))
    print(f"wrote {name}.npz: {len(raised)} queries, {int((raised != 0).sum())} raised "
          f"({int((raised == 1).sum())} NetworkXNoPath, {int((raised == 2).sum())} NodeNotFound)")
