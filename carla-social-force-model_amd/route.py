"""Routes over walk graphs: the packer of ``SfmBatch.set_routes`` and the NumPy twins of sfm_batch_plan_routes_kernel
(csrc/sfm_batch_route.hip).  Pure NumPy; the rule is specified in include/sfm_hip.h (routes) and DESIGN.md section 3.7p.

What it restates is the reference's ``path_planner.PedPathPlanner.generate_route`` -- shortest path over a sidewalk / crosswalk /
jaywalking graph, three sub-graphs selected by edge type (``_extract_subgraphs``), jaywalking edges made dearer by a weight factor
(``_add_topology_edges_to_graph``), first and last node dropped when they would be a detour
(``_remove_unnecessary_start_end_nodes``), the destination appended -- as a rule that is a pure function of the graph, bit for
bit in fp32: distances from the end node in synchronous rounds, every round reading the round before only.  The graph is the
caller's; building it from a map is not part of this package.

One departure: the reference finds the end nodes through the CARLA lane a location lies in; here they are the usable nodes nearest
to the origin and to the goal.  Where the reference finds a node that is in the row's sub-graph at all, it is the nearest one.
"""
from __future__ import annotations

import numpy as np

from .scan import _fma32

SIDEWALK, CROSSWALK, JAYWALKING, JAYWALKING_JUNCTION, SIDEWALK_TO_ROAD = 1, 2, 3, 4, 5     # path_planner.EdgeType
NO_JAYWALKING, JAYWALKING_AT_JUNCTION, JAYWALKING_ANYWHERE = 1, 2, 3                        # path_planner.GraphType
MAX_NODES = 1024                  # SFM_BATCH_MAX_ROUTE_NODES
MAX_CAPACITY = 64                 # SFM_BATCH_MAX_ROUTE_CAPACITY
STATUS_NONE, STATUS_PLANNED, STATUS_NO_PATH, STATUS_TOO_LONG, STATUS_NOT_LIVE, STATUS_BAD_GOAL = 0, 1, 2, 3, 4, 5
NEAR_LIMIT = np.float32(1.0e12)   # a live row: |x|, |y| below it (sfm_device.h)
MODE_WALKING, MODE_DESPAWNED = 1, 255
_DROPPED = {NO_JAYWALKING: (3, 4, 5), JAYWALKING_AT_JUNCTION: (3, 5), JAYWALKING_ANYWHERE: ()}
_F = np.float32


def kept(types, g):
    """bool per edge type value: does the sub-graph of graph type ``g`` keep it (path_planner._extract_subgraphs)"""
    if int(g) not in _DROPPED:
        raise ValueError(f"graph type must be 1, 2 or 3, got {g}")
    return ~np.isin(np.asarray(types), _DROPPED[int(g)])


def pack_graph(graph, scene=0):
    """One scene's graph dict -> its CSR adjacency: ``dict(xy (V,2) f32, off (V+1,) i32, nbr (A,) i32, w (A,) f32, typ (A,) u8)``
    with each node's neighbours in ascending index, or None for ``graph=None``.  Keys of ``graph``: ``nodes`` (V, 2|3), ``edges``
    (E, 2), ``types`` (E,) EdgeType values 1..5, and optionally ``lengths`` (E,) and ``jaywalking_weight_factor`` (default 2).  A
    duplicate edge overrides the one given before it, as ``nx.Graph.add_edge`` does.  Raises ValueError naming scene and key."""
    if graph is None:
        return None
    where = f"scene {scene}: "
    for key in ("nodes", "edges", "types"):
        if key not in graph:
            raise ValueError(where + f"the graph has no '{key}'")
    unknown = set(graph) - {"nodes", "edges", "types", "lengths", "jaywalking_weight_factor"}
    if unknown:
        raise ValueError(where + f"unknown graph key(s) {sorted(unknown)}")
    nodes = np.asarray(graph["nodes"], dtype=np.float64)
    if nodes.ndim != 2 or nodes.shape[1] not in (2, 3):
        raise ValueError(where + f"nodes must have shape (V, 2) or (V, 3), got {nodes.shape}")
    V = nodes.shape[0]
    if V > MAX_NODES:
        raise ValueError(where + f"nodes: {V} nodes, at most {MAX_NODES} per scene")
    if not np.isfinite(nodes[:, :2]).all():
        raise ValueError(where + "nodes must be finite")
    edges = np.asarray(graph["edges"])
    if edges.size == 0:
        edges = np.zeros((0, 2), np.int64)
    if edges.ndim != 2 or edges.shape[1] != 2 or edges.dtype.kind not in "iu":
        raise ValueError(where + f"edges must be integers of shape (E, 2), got {edges.dtype} {edges.shape}")
    edges = edges.astype(np.int64)
    E = edges.shape[0]
    if E and (edges.min() < 0 or edges.max() >= V):
        k = int(np.flatnonzero((edges < 0).any(1) | (edges >= V).any(1))[0])
        raise ValueError(where + f"edges[{k}] = {tuple(int(v) for v in edges[k])} is out of range for {V} nodes")
    if E and (edges[:, 0] == edges[:, 1]).any():
        k = int(np.flatnonzero(edges[:, 0] == edges[:, 1])[0])
        raise ValueError(where + f"edges[{k}] is a self loop on node {int(edges[k, 0])}")
    types = np.asarray(graph["types"])
    if types.shape != (E,) or (E and types.dtype.kind not in "iu"):
        raise ValueError(where + f"types must be {E} integers, got {types.dtype} {types.shape}")
    types = types.astype(np.int64)
    if E and ((types < 1) | (types > 5)).any():
        k = int(np.flatnonzero((types < 1) | (types > 5))[0])
        raise ValueError(where + f"types[{k}] = {int(types[k])}: an EdgeType value 1..5 (VOID, -1, is no edge)")
    if graph.get("lengths") is None:
        d = nodes[edges[:, 0], :2] - nodes[edges[:, 1], :2]
        lengths = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    else:
        lengths = np.asarray(graph["lengths"], dtype=np.float64)
        if lengths.shape != (E,):
            raise ValueError(where + f"lengths must hold {E} values, got shape {lengths.shape}")
    if E and not (np.isfinite(lengths) & (lengths >= 0)).all():
        k = int(np.flatnonzero(~(np.isfinite(lengths) & (lengths >= 0)))[0])
        raise ValueError(where + f"lengths[{k}] = {lengths[k]}: must be finite and >= 0")
    factor = float(graph.get("jaywalking_weight_factor", 2.0))
    if not np.isfinite(factor) or factor < 0:
        raise ValueError(where + f"jaywalking_weight_factor = {factor}: must be finite and >= 0")
    with np.errstate(over="ignore"):
        len32 = lengths.astype(_F)
        w = np.where((types == JAYWALKING) | (types == JAYWALKING_JUNCTION), len32 * _F(factor), len32).astype(_F)
    if E and not np.isfinite(w).all():
        k = int(np.flatnonzero(~np.isfinite(w))[0])
        raise ValueError(where + f"lengths[{k}]: the weight does not fit float32")
    # the last edge given between two nodes wins
    lo, hi = edges.min(1) if E else edges[:, 0], edges.max(1) if E else edges[:, 0]
    key = lo * V + hi
    _, last = np.unique(key[::-1], return_index=True)
    keep = np.sort(E - 1 - last)
    a = np.concatenate([edges[keep, 0], edges[keep, 1]])
    bq = np.concatenate([edges[keep, 1], edges[keep, 0]])
    order = np.lexsort((bq, a))
    off = np.zeros(V + 1, np.int32)
    np.cumsum(np.bincount(a, minlength=V), out=off[1:])
    return {"xy": np.ascontiguousarray(nodes[:, :2], dtype=_F), "off": off, "nbr": bq[order].astype(np.int32),
            "w": np.concatenate([w[keep], w[keep]])[order].astype(_F), "typ": np.concatenate([types[keep], types[keep]])[order].astype(np.uint8)}


def pack_graphs(graphs):
    """A list of B graph dicts (``None``: the scene has no routes) -> what sfm_batch_set_routes takes, concatenated over the scenes:
    ``node_off`` [B+1], ``node_x`` / ``node_y``, ``adj_off`` [V_total+1] (into the adjacency arrays), ``adj_node`` (scene-local),
    ``adj_w``, ``adj_type``; and ``scenes``, the per-scene ``pack_graph`` outputs the twins take."""
    per = [pack_graph(g, k) for k, g in enumerate(graphs)]
    V = [0 if p is None else p["xy"].shape[0] for p in per]
    node_off = np.zeros(len(per) + 1, np.int32)
    np.cumsum(V, out=node_off[1:])
    live = [p for p in per if p is not None]
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([p[k] for p in live]) if live else np.zeros(0), dtype=dt)
    xy = np.concatenate([p["xy"] for p in live]) if live else np.zeros((0, 2), _F)
    adj_off, base = [np.zeros(1, np.int64)], 0
    for p in live:
        adj_off.append(p["off"][1:].astype(np.int64) + base)
        base += int(p["off"][-1])
    if base >= 2 ** 31:
        raise ValueError("the graphs hold more than 2^31 - 1 adjacency entries")
    return {"node_off": node_off, "node_x": np.ascontiguousarray(xy[:, 0]), "node_y": np.ascontiguousarray(xy[:, 1]),
            "adj_off": np.concatenate(adj_off).astype(np.int32), "adj_node": cat("nbr", np.int32), "adj_w": cat("w", _F),
            "adj_type": cat("typ", np.uint8), "scenes": per}


def usable_nodes(graph, g):
    """bool (V,): the nodes at least one kept edge of graph type ``g`` touches (``graph``: a ``pack_graph`` output)"""
    k = kept(graph["typ"], g)
    V = graph["xy"].shape[0]
    src = np.repeat(np.arange(V), np.diff(graph["off"]))
    return np.bincount(src[k], minlength=V) > 0


def d2(a, b):
    """fmaf(dx, dx, dy * dy) on fp32 differences, the kernel's squared distance (``scan._fma32`` is an exact fmaf)"""
    a, b = np.asarray(a, _F), np.asarray(b, _F)
    dx, dy = (a[..., 0] - b[..., 0]).astype(_F), (a[..., 1] - b[..., 1]).astype(_F)
    with np.errstate(over="ignore", invalid="ignore"):
        yy = (dy * dy).astype(_F)
        return _fma32(dx, dx, yy)


def _nearest(xy, ok, p):
    """the usable node nearest to p: strict <, ascending, so the lowest index wins a tie; -1 when none is nearer than +inf"""
    if not ok.any():
        return -1
    dist = np.where(ok, d2(xy, np.asarray(p, _F)[None, :]), _F(np.inf))
    dist = np.where(np.isnan(dist), _F(np.inf), dist)
    j = int(np.argmin(dist))                                          # (first occurrence of the minimum)
    return j if dist[j] < np.inf else -1


def distance_field(graph, g, t):
    """(D (V,) f32, nxt (V,) i32 adjacency slot or -1, rounds): distances from node ``t`` over the kept edges of graph type ``g``
    in synchronous rounds -- D_r[v] = min(D_{r-1}[v], min over kept (v, u) of fl(D_{r-1}[u] + w)), nxt[v] the lowest u among the
    strict improvements' minima -- until a round changes nothing, at most V rounds."""
    V = graph["xy"].shape[0]
    off, nbr, w = graph["off"], graph["nbr"], graph["w"]
    keep = kept(graph["typ"], g)
    deg = np.diff(off)
    width = max(int(deg.max()) if V else 0, 1)
    slot = off[:-1, None].astype(np.int64) + np.arange(width)[None, :]
    valid = np.arange(width)[None, :] < deg[:, None]
    slot = np.where(valid, slot, 0)
    valid &= keep[slot] if nbr.size else False
    U = np.where(valid, nbr[slot] if nbr.size else 0, 0)
    W = np.where(valid, w[slot] if nbr.size else 0, _F(np.inf)).astype(_F)
    D = np.full(V, np.inf, _F)
    D[t] = 0
    nxt = np.full(V, -1, np.int64)
    rows = np.arange(V)
    rounds = 0
    for _ in range(V):
        rounds += 1
        with np.errstate(over="ignore"):
            cand = (D[U] + W).astype(_F)                              # one fp32 add per candidate (inf where there is no edge)
        j = np.argmin(cand, axis=1)                                   # first minimum: neighbours ascend, the lowest u wins
        best = cand[rows, j]
        better = best < D
        if not better.any():
            break
        nxt = np.where(better, slot[rows, j], nxt)
        D = np.where(better, best, D)
    return D, nxt.astype(np.int32), rounds


def plan_row(graph, g, origin, goal, capacity=MAX_CAPACITY, field=None):
    """One row's route, the twin of one wave of the kernel: dict(status, s, t, cost, L, xy (L, 2) f32, cross (L,) u8, nodes) with
    status 1 (planned), 2 (no usable node, or t not reachable from s: the row walks straight, L = 1), 3 (L - 1 > capacity: likewise)
    or 5 (goal not finite: nothing).  ``graph``: a ``pack_graph`` output; ``origin``, ``goal``: (2|3,), z ignored; ``nodes``: the
    untrimmed node sequence s .. t.  ``field``: a dict the distance fields are cached in per (t, g)."""
    o = np.asarray(origin, dtype=np.float64)[:2].astype(_F)
    with np.errstate(over="ignore"):
        d = np.asarray(goal, dtype=np.float64)[:2].astype(_F)
    straight = {"s": -1, "t": -1, "cost": _F(np.inf), "L": 1, "xy": d[None, :].copy(), "cross": np.zeros(1, np.uint8), "nodes": []}
    if not np.isfinite(d).all():
        return {**straight, "status": STATUS_BAD_GOAL, "L": 0, "xy": np.zeros((0, 2), _F), "cross": np.zeros(0, np.uint8)}
    if graph is None or graph["xy"].shape[0] == 0:
        return {**straight, "status": STATUS_NO_PATH}
    xy = graph["xy"]
    V = xy.shape[0]
    ok = usable_nodes(graph, g)
    s, t = _nearest(xy, ok, o), _nearest(xy, ok, d)
    if s < 0 or t < 0:
        return {**straight, "status": STATUS_NO_PATH, "s": s, "t": t}
    key = (int(t), int(g))
    if field is not None and key in field:
        D, nxt = field[key]
    else:
        D, nxt, _ = distance_field(graph, g, t)
        if field is not None:
            field[key] = (D, nxt)
    if not np.isfinite(D[s]):
        return {**straight, "status": STATUS_NO_PATH, "s": s, "t": t}
    nodes, etype, v = [s], [], s
    for _ in range(V - 1):                                            # walk next from s to t, at most V - 1 hops (no cycle: no more)
        if v == t:
            break
        e = int(nxt[v])
        if e < 0:
            break
        etype.append(int(graph["typ"][e]))
        v = int(graph["nbr"][e])
        nodes.append(v)
    if v != t:
        return {**straight, "status": STATUS_NO_PATH, "s": s, "t": t}
    a, b = 0, len(nodes) - 1
    if len(nodes) > 1:                                                # both tests on the untrimmed list
        drop_first = d2(xy[nodes[0]], xy[nodes[1]]) > d2(o, xy[nodes[1]])
        drop_last = d2(xy[nodes[-1]], xy[nodes[-2]]) > d2(d, xy[nodes[-2]])
        a += int(drop_first)
        b -= int(drop_last)
    pts, flags = [], []
    if b - a + 1 >= 2:
        for j in range(a, b + 1):
            pts.append(xy[nodes[j]])
            flags.append(0 if j == a else int(etype[j - 1] in (CROSSWALK, JAYWALKING, JAYWALKING_JUNCTION)))
    pts.append(d)
    flags.append(0)
    L = len(pts)
    out = {"s": s, "t": t, "cost": _F(D[s]), "nodes": nodes}
    if L - 1 > int(capacity):
        return {**straight, **out, "status": STATUS_TOO_LONG, "L": L}
    return {**out, "status": STATUS_PLANNED, "L": L, "xy": np.asarray(pts, _F).reshape(L, 2), "cross": np.asarray(flags, np.uint8)}


def plan_scene(graph, graph_types, positions, goals, capacity=16, modes=None):
    """A scene's rows, the twin of one workgroup: ``graph_types`` (N,) with 0 for a row that is not routed, ``positions`` and
    ``goals`` (N, 2|3), ``modes`` (N,) PedMode values (255: despawned) or None.  Returns one entry per row: None for an unrouted
    row, else ``plan_row``'s dict -- with status 4 and nothing else for a row that is not live."""
    gt = np.asarray(graph_types)
    pos = np.asarray(positions, dtype=np.float64)
    with np.errstate(over="ignore"):
        p32 = pos[:, :2].astype(_F)
    field, out = {}, []
    for i in range(gt.shape[0]):
        if int(gt[i]) == 0:
            out.append(None)
            continue
        live = bool(abs(p32[i, 0]) < NEAR_LIMIT and abs(p32[i, 1]) < NEAR_LIMIT)
        if not live or (modes is not None and int(modes[i]) == MODE_DESPAWNED):
            out.append({"status": STATUS_NOT_LIVE, "s": -1, "t": -1, "cost": _F(np.inf), "L": 0, "xy": np.zeros((0, 2), _F),
                        "cross": np.zeros(0, np.uint8), "nodes": []})
            continue
        out.append(plan_row(graph, int(gt[i]), pos[i], np.asarray(goals)[i], capacity, field))
    return out


def queue_slots(plan, capacity):
    """(xy (capacity, 2) f32 with NaN in the unused slots' place left out, cursor): where the kernel leaves entries 1 .. L-1 --
    right-aligned in slots [capacity - (L - 1), capacity).  Returns (first used slot = cursor, xy (L-1, 2), cross (L-1,))."""
    L = int(plan["L"]) if plan["status"] == STATUS_PLANNED else 1
    return int(capacity) - (L - 1), plan["xy"][1:L], plan["cross"][1:L]
