"""The batch shared by the vehicle-scan tests (test_batch_vehicle_scan_host.py, test_batch_vehicle_scan_gpu.py): the scenes, the
masks, and the index arithmetic of the kernel's tiles and shares restated on the host, so that the host file can assert what the
batch holds and the GPU file runs exactly that batch."""
import copy
from functools import lru_cache

import numpy as np

from carla_social_force_model_amd import scan as S, scenarios

TILE, WAVE = 512, 64                                  # sfm_batch_vehicle_scan.hip: points per LDS tile, lanes per wave
SIZES = (17, 0, 1, 17, 64, 65, 300, 1024, 17)         # pedestrians per scene
COUNTS = (0, 2, 1, 2, 3, 5, 9, 2, 3)                  # vehicles per scene
RMAX = [6.0, 9.0, 5.0, 7.0, 6.0, 8.0, 6.5, 5.0, 12.0]
PED = [0.3, 0.3, 0.25, 0.4, 0.3, 0.35, 0.3, 0.3, 0.3]
POINT = [0.1, 0.15, 0.1, 0.1, 0.2, 0.1, 0.1, 0.1, 0.1]
DTS = [0.05, 0.04, 0.02, 0.05, 0.03, 0.05, 0.05, 0.04, 0.05]
MOUNT = (1.25, -0.5)
RAYS = (1, 8, 33, 64, 65, 256)
GHOST, NAN_ROW = 3, 7                                 # rows of scene 5
ABSENT = (6, 4)                                       # (scene, vehicle): tracked, first tick 40
# which vehicles are scanned: per name one entry per scene; "all" is no mask at all (a NULL pointer for the library)
MASKS = {"all": [None] * 9,
         "first": [[], [1, 0], [1], [1, 0], [1, 0, 0], [1, 0, 0, 0, 0], [1] + [0] * 8, [1, 0], [1, 0, 0]],
         "middle": [[], [0, 1], [1], [0, 1], [0, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 1, 0, 0, 0], [0, 1], [0, 1, 0]],
         "last": [[], [0, 1], [1], [0, 1], [0, 0, 1], [0, 0, 0, 0, 1], [0] * 8 + [1], [1, 1], [0, 0, 1]]}

ZERO = (0.0, 0.0)
# what the GPU file runs -- R, frame, mount, mask, planar: every R with both frames, both mounts, every mask and both uploads somewhere
CASES = [(1, 0, ZERO, "all", None), (1, 1, MOUNT, "middle", None), (8, 1, MOUNT, "first", None), (8, 0, ZERO, "all", False),
         (33, 0, MOUNT, "middle", False), (33, 1, ZERO, "all", None), (64, 1, ZERO, "last", None), (64, 0, MOUNT, "first", None),
         (65, 1, MOUNT, "first", False), (65, 0, ZERO, "middle", None), (256, 0, MOUNT, "all", None), (256, 1, ZERO, "last", False)]


def mask_arg(name):
    """The mask as set_vehicle_scan takes it."""
    return None if name == "all" else MASKS[name]


def fan(R):
    """R ray angles: a forward fan of 240 degrees (one ray: straight ahead)."""
    return np.zeros(1) if R == 1 else np.linspace(-2.0 * np.pi / 3.0, 2.0 * np.pi / 3.0, R)


def _trim_borders(sc, t):
    """Takes the last t border points out of the scene (whole polylines while fewer than two points would stay)."""
    while t > 0:
        last = sc["borders"][-1]
        if len(last) - t >= 2:
            sc["borders"][-1] = last[:-t]
            return
        t -= len(last)
        sc["borders"] = sc["borders"][:-1]
        sc["border_centers"], sc["border_lengths"] = sc["border_centers"][:-1], sc["border_lengths"][:-1]


def counts(sc):
    """(border points, static points, ring sizes) of a scene."""
    return (sum(len(p) for p in sc["borders"]), sum(len(r) for _, r in sc["static_obstacles"]),
            [len(r) for _, r in sc["dynamic_obstacles"]])


def own_ring(sc, k):
    """Vehicle k's own ring as [lo, hi) of the geometry's virtual run (borders, static points, rings)."""
    nb, ns, rings = counts(sc)
    lo = nb + ns + sum(rings[:k])
    return lo, lo + rings[k]


def straddles_tile(sc, k):
    lo, hi = own_ring(sc, k)
    return any(lo < m < hi for m in range(TILE, hi, TILE))


def split_of(items):
    return 4 if items <= WAVE else 2 if items <= 2 * WAVE else 1


def straddles_share(sc, k, split, point_radius):
    """Whether a boundary between two waves' shares of the fixed order falls strictly inside vehicle k's own ring."""
    nb, ns, rings = counts(sc)
    n, G = len(sc["loc"]), (nb + ns + sum(rings) if point_radius > 0 else 0)
    lo, hi = own_ring(sc, k)
    return G > 0 and any(n + lo < (n + G) * s // split < n + hi for s in range(1, split))


@lru_cache(maxsize=None)
def _made():
    import test_batch_gpu as TB
    import test_batch_tracks_gpu as TR
    import test_batch_vehicles_gpu as V
    scenes = []
    for k, (n, m) in enumerate(zip(SIZES, COUNTS)):
        sc = TB._scene(n, 4200 + k, geo=k != 1, dynamic=m)
        rng = np.random.default_rng(900 + k)
        if m and n:                                                       # the vehicles stand inside the crowd
            c = np.float32(sc["loc"][rng.integers(0, n, m), :2] + rng.uniform(-1.5, 1.5, (m, 2))).astype(np.float64)
            sc["dynamic_obstacles"] = [(c[j], sc["dynamic_obstacles"][j][1]) for j in range(m)]
        elif m:                                                           # no crowd: two vehicles in sight of each other
            c = np.array([[2.0, 3.0], [6.0, 4.0]])
            sc["dynamic_extent"] = np.array([[3.0, 1.2], [1.6, 0.8]])     # unequal rings: the middle of the run lies inside ring 0
            sc["dynamic_obstacles"] = [(c[j], sc["dynamic_obstacles"][j][1]) for j in range(m)]
        sc["dynamic_vel"] = np.float32(sc["dynamic_vel"] * 0.1).astype(np.float64)
        V._restart_twin(sc)
        scenes.append(sc)
    sc = scenes[5]
    sc["loc"][GHOST, :2] = (3.0e15, -3.0e15)
    sc["vel"][GHOST] = 0.0
    sc["loc"][NAN_ROW, :2] = np.nan
    # scene 8: more than TILE points in front of the rings, cut so that vehicle 0's own ring lies across a tile boundary
    sc = scenes[8]
    nb, ns, rings = counts(sc)
    assert nb + ns >= TILE, "scene 8 needs more geometry: choose another seed"
    _trim_borders(sc, (nb + ns) % TILE + rings[0] // 2)
    rng = np.random.default_rng(77)
    tracks = [None] * len(scenes)
    tracks[ABSENT[0]] = [None] * COUNTS[ABSENT[0]]
    tracks[ABSENT[0]][ABSENT[1]] = TR._track(rng, 5, 40, TR._mid(scenes[ABSENT[0]]))
    cfgs = [TB._config(k, scenarios.ALL_FORCES) for k in range(len(scenes))]
    return scenes, cfgs, tracks


def made(finite=False):
    """(scenes, configs, tracks), fresh copies; the twin of the batch as it is after upload(device_vehicles=True) and
    set_vehicle_tracks(tracks).  ``finite``: the NaN row is parked like the ghost (for tests that run ticks)."""
    import _driving_cases as D
    scenes, cfgs, tracks = copy.deepcopy(_made())
    if finite:
        scenes[5]["loc"][NAN_ROW, :2] = (3.0e15, 3.0e15)
    D.start_twin(scenes, tracks)
    return scenes, cfgs, tracks


def twin(scenes, R, frame, mount, mask, state=None):
    """The record of every scene from the twin: a list of (M_b, 2R) arrays."""
    return [S.scan_vehicles_scene(sc, fan(R), RMAX[s], PED[s], POINT[s], frame=frame, mask=MASKS[mask][s], mount=mount,
                                  state=None if state is None else state[s]) for s, sc in enumerate(scenes)]


def scanned(scenes, mask):
    """Per scene the indices of the vehicles that are scanned and present."""
    out = []
    for s, sc in enumerate(scenes):
        m = MASKS[mask][s]
        want = np.ones(len(sc["dynamic_obstacles"]), bool) if m is None else np.asarray(m, bool)
        present = np.asarray(sc.get("dynamic_present", np.ones(len(want), bool)), bool)
        out.append(np.flatnonzero(want & present))
    return out
