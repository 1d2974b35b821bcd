"""Walk graphs and route queries shared by the route tests (tests/test_batch_routes_host.py, tests/test_batch_routes_gpu.py) and
by tests/golden/make_golden_routes.py, which feeds them to the reference's own planner.  Inputs are generated here and never
stored; the fixtures hold the reference's answers and the SHA-256 of the inputs they were made from.

The reference keys a node on its coordinates rounded to 0 decimals (path_planner._generate_edge_dicts), so every graph that goes
to the reference keeps its nodes at least 2 m apart around distinct integers.

Rounding bounds.  The rule under test is fp32, the reference float64.  A float64 decision may be left out of the comparison only
when it lies inside what fp32 can move it by; EPS = 2^-24 is half an fp32 ulp, relative.
  * Path costs: an edge weight is rounded to fp32 (EPS), a jaywalking weight once more by the factor's product (EPS), and each of
    the h adds of a path of h hops rounds once (EPS of a partial sum <= the cost): a path's fp32 cost is within (h + 2) EPS cost of
    its float64 cost.  Two paths can therefore change order only when their float64 costs differ by at most
    2 (h + 2) EPS cost (``path_bound``), h the larger hop count and cost the larger cost.
  * Squared distances: a coordinate rounds to fp32 (EPS |c|), the difference rounds once more (EPS |dx|), so dx carries an absolute
    error ex <= EPS (|a.x| + |b.x| + |dx|); d2 = fmaf(dx, dx, dy * dy) adds two roundings, of dy * dy and of the sum (2 EPS d2):
    |err d2| <= 2 (|dx| ex + |dy| ey) + ex^2 + ey^2 + 2 EPS d2  (``d2_bound``).  A comparison of two squared distances is left out
    only when they differ by at most the sum of their bounds.
"""
import hashlib

import numpy as np

EPS = 2.0 ** -24
SIDEWALK, CROSSWALK, JAYWALKING, JAYWALKING_JUNCTION, SIDEWALK_TO_ROAD = 1, 2, 3, 4, 5


def path_bound(hops, cost):
    return 2.0 * (hops + 2) * EPS * cost


def d2_bound(a, b):
    a, b = np.asarray(a, np.float64)[:2], np.asarray(b, np.float64)[:2]
    d = np.abs(a - b)
    e = EPS * (np.abs(a) + np.abs(b) + d)
    dist2 = float(d @ d)
    return float(2.0 * (d @ e) + e @ e + 2.0 * EPS * dist2)


def d2_64(a, b):
    d = np.asarray(a, np.float64)[:2] - np.asarray(b, np.float64)[:2]
    return float(d @ d)


# ---- graphs ------------------------------------------------------------------------------------------------------------------
def grid_edges(kx, ky):
    e = []
    for i in range(ky):
        for j in range(kx):
            v = i * kx + j
            if j + 1 < kx:
                e.append((v, v + 1))
            if i + 1 < ky:
                e.append((v, v + kx))
    return np.asarray(e, dtype=np.int64).reshape(-1, 2)


def street_grid(kx, ky, seed, spacing=10.0, jitter=2.0, types=None, factor=2.0):
    """A jittered kx x ky street grid with random edge types (or ``types``: one value for every edge)."""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.arange(kx) * spacing, np.arange(ky) * spacing)
    nodes = np.stack([xs.ravel(), ys.ravel()], axis=1) + rng.uniform(-jitter, jitter, (kx * ky, 2))
    edges = grid_edges(kx, ky)
    # (mostly sidewalks, as a street map is: with the five types equally likely the sub-graphs fall apart and the reference raises
    #  on four queries in ten)
    t = rng.choice([1, 2, 3, 4, 5], len(edges), p=[0.7, 0.12, 0.06, 0.08, 0.04]) if types is None else np.full(len(edges), types, dtype=np.int64)
    return {"nodes": nodes, "edges": edges, "types": t, "jaywalking_weight_factor": factor}


def integer_grid(k, spacing=3.0):
    """k x k nodes on exact multiples of ``spacing``, sidewalks only: every monotone staircase between two nodes costs the same."""
    xs, ys = np.meshgrid(np.arange(k) * spacing, np.arange(k) * spacing)
    edges = grid_edges(k, k)
    return {"nodes": np.stack([xs.ravel(), ys.ravel()], axis=1), "edges": edges, "types": np.ones(len(edges), np.int64)}


def chain(V, spacing=3.0, types=SIDEWALK):
    nodes = np.stack([np.arange(V) * spacing, np.zeros(V)], axis=1)
    edges = np.stack([np.arange(V - 1), np.arange(1, V)], axis=1).reshape(-1, 2)
    return {"nodes": nodes, "edges": edges, "types": np.full(len(edges), types, dtype=np.int64)}


def star(V, radius=40.0):
    """node 0 in the middle, V - 1 leaves on a circle; the leaves' edges alternate sidewalk and crosswalk"""
    a = np.arange(V - 1) * (2.0 * np.pi / max(V - 1, 1))
    nodes = np.concatenate([np.zeros((1, 2)), radius * np.stack([np.cos(a), np.sin(a)], axis=1)])
    edges = np.stack([np.zeros(V - 1, np.int64), np.arange(1, V)], axis=1)
    return {"nodes": nodes, "edges": edges, "types": 1 + (np.arange(V - 1) % 2)}


def two_components():
    """two sidewalk squares 100 m apart, no edge between them"""
    sq = np.array([[0.0, 0.0], [6.0, 0.0], [6.0, 6.0], [0.0, 6.0]])
    ring = np.array([[0, 1], [1, 2], [2, 3], [3, 0]])
    return {"nodes": np.concatenate([sq, sq + [100.0, 0.0]]), "edges": np.concatenate([ring, ring + 4]), "types": np.ones(8, np.int64)}


def three_ways(factor=2.0):
    """From node 0 to node 1 across a road: a jaywalking edge straight across (20 m, reached over two sidewalk-to-road stubs),
    a junction 30 m up the road (jaywalking at the junction) and a crosswalk 60 m up.  The three graph types give three routes.
        0 -2- 6 ..jay.. 7 -2- 1          (6, 7: the kerbs; stubs of type 5)
        |                    |
        2 ....junction...... 3           (30 m up, type 4)
        |                    |
        4 ====crosswalk===== 5           (60 m up, type 2)"""
    nodes = np.array([[0.0, 0.0], [24.0, 0.0], [0.0, 30.0], [24.0, 30.0], [0.0, 60.0], [24.0, 60.0], [2.0, 0.0], [22.0, 0.0]])
    edges = np.array([[0, 2], [2, 4], [1, 3], [3, 5], [4, 5], [2, 3], [0, 6], [7, 1], [6, 7]])
    types = np.array([1, 1, 1, 1, CROSSWALK, JAYWALKING_JUNCTION, SIDEWALK_TO_ROAD, SIDEWALK_TO_ROAD, JAYWALKING])
    return {"nodes": nodes, "edges": edges, "types": types, "jaywalking_weight_factor": factor}


def random_graph(V, seed, extra=1.5, spacing=4.0):
    """V nodes on a jittered lattice (>= 2 m apart around distinct integers), a random spanning tree plus ``extra`` V more edges"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(V)))
    cells = rng.permutation(side * side)[:V]
    nodes = np.stack([cells % side, cells // side], axis=1) * spacing + rng.uniform(-0.4, 0.4, (V, 2))
    e = [(int(rng.integers(0, v)), v) for v in range(1, V)]
    for _ in range(int(extra * V)):
        a, b = rng.integers(0, V, 2)
        if a != b:
            e.append((int(a), int(b)))
    edges = np.asarray(e, dtype=np.int64).reshape(-1, 2)
    return {"nodes": nodes, "edges": edges, "types": rng.integers(1, 6, len(edges))}


# ---- the cases that go to the reference -------------------------------------------------------------------------------------
def reference_sets():
    """name -> list of (graph, [(origin (3,), goal (3,), graph_type), ...]).  ``random``: 40 jittered street grids of 2x2 .. 6x6
    nodes with random edge types and 20 queries each; ``designed``: the hand-built graphs with queries that meet every branch."""
    rng = np.random.default_rng(2300)
    rnd = []
    for k in range(40):
        side = 2 + k % 5
        g = street_grid(side, side, 2310 + k)
        span = 10.0 * (side - 1)
        q = [(np.append(rng.uniform(-5.0, span + 5.0, 2), 0.0), np.append(rng.uniform(-5.0, span + 5.0, 2), 0.0), int(rng.integers(1, 4)))
             for _ in range(20)]
        rnd.append((g, q))
    z = lambda x, y: np.array([x, y, 0.0])
    designed = []
    ig = integer_grid(5)
    designed.append((ig, [(z(0.4, 0.3), z(12.3, 11.6), 1), (z(11.8, 0.2), z(0.3, 12.4), 3), (z(6.2, 5.9), z(6.4, 6.1), 2),      # ties; s == t
                          (z(-1.0, -1.2), z(13.1, 12.9), 1)]))
    ch = chain(6, spacing=5.0)
    designed.append((ch, [(z(2.0, 0.5), z(23.0, -0.5), 1),          # both ends trimmed: the origin lies past node 0 towards node 1
                          (z(2.0, 0.5), z(26.0, 0.3), 1),           # the first only
                          (z(-1.0, 0.2), z(23.0, 0.4), 1),          # the last only
                          (z(-1.0, 0.2), z(26.0, 0.3), 1),          # neither
                          (z(1.0, 0.1), z(4.0, 0.1), 1),            # a two-node route with both nodes trimmed
                          (z(11.0, 0.3), z(9.0, -0.3), 2)]))        # s == t
    for f in (2.0, 1.0, 4.0):                                       # (a factor that flips the route: 1 makes the junction cheapest)
        designed.append((three_ways(f), [(z(-0.5, -0.5), z(24.5, -0.5), g) for g in (1, 2, 3)] +
                         [(z(0.5, 29.0), z(24.5, 31.0), g) for g in (1, 2, 3)]))
    designed.append((two_components(), [(z(1.0, 1.0), z(104.0, 5.0), 1), (z(1.0, 1.0), z(5.0, 5.5), 1)]))   # no path; a path
    return {"random": rnd, "designed": designed}


def digest(cases):
    h = hashlib.sha256()
    for g, queries in cases:
        for key in ("nodes", "edges", "types"):
            a = np.ascontiguousarray(g[key], dtype=np.float64 if key == "nodes" else np.int64)
            h.update(key.encode() + str(a.shape).encode() + a.tobytes())
        h.update(np.float64(g.get("jaywalking_weight_factor", 2.0)).tobytes())
        for o, d, t in queries:
            h.update(np.asarray(o, np.float64).tobytes() + np.asarray(d, np.float64).tobytes() + np.int64(t).tobytes())
    return h.hexdigest()
