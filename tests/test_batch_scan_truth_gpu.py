"""GPU tests that hold the range scan's DEVICE record to the float64 ray cast of ``_scan_truth`` -- no twin in between -- and take
the kernel through the regimes and boundaries its first tests left out: long ranges, radii of a millimetre and of 25 m, directions
that are not unit vectors, the zero direction, and item counts, geometry counts, kind boundaries and wave shares chosen against the
kernel's own cuts (256 items per pass, 4 / 2 waves per item up to 64 / 128 items, LDS tiles of 512 points).  What a scene is built
to contain is asserted from the scene and the float64 reference before the device is looked at."""
from functools import lru_cache

import numpy as np
import pytest

import _scan_truth as T
import test_batch_gpu as G
import test_batch_scan_gpu as SG
from carla_social_force_model_amd.batch import pack_scenes
from carla_social_force_model_amd.scan import default_angles, ray_directions, scan_scene

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 64, 65, 129, 257, 1024)
RMAX = (20.0, 6.0, 10.0)                                                # per scene, in turn
PED = (0.3, 0.45, 0.2)
POINT = (0.1, 0.25, 0.1)
TILE, ITEMS_4, ITEMS_2 = 512, 64, 128                                   # SCAN_TILE; up to 64 (128) items 4 (2) waves share one


def _settings(B):
    return [RMAX[b % 3] for b in range(B)], [PED[b % 3] for b in range(B)], [POINT[b % 3] for b in range(B)]


@lru_cache(maxsize=None)
def _scenes(far=False, z3=False):
    scenes = [G._scene(n, 7100 + q, dynamic=3) for q, n in enumerate(SIZES)]
    if far:
        scenes = [T.shifted(sc) for sc in scenes]
    if z3:
        rng = np.random.default_rng(5)
        for sc in scenes:
            n = len(sc["loc"])
            sc["loc"] = np.column_stack([np.asarray(sc["loc"])[:, :2], rng.uniform(0.0, 1.5, n)])
            sc["vel"] = np.column_stack([np.asarray(sc["vel"])[:, :2], rng.uniform(-0.2, 0.2, n)])
    return scenes


@lru_cache(maxsize=None)
def _masks():
    """Every row of every scene, but 37 rows of the 1 024-row scene: the first and last row of a wave, of a pass and of the scene,
    and 30 more."""
    masks = [np.ones(n, bool) for n in SIZES]
    masks[-1] = np.zeros(1024, bool)
    masks[-1][[0, 63, 64, 255, 256, 257, 1023]] = True
    masks[-1][5::34] = True
    assert masks[-1].sum() == 37
    return masks


@lru_cache(maxsize=None)
def _pack(far):
    return pack_scenes(_scenes(far))


@lru_cache(maxsize=None)
def _device(R, frame, far, z3):
    return SG._scanned(_scenes(far, z3), *_settings(len(SIZES)), R=R, frame=frame, mask=list(_masks()))


@lru_cache(maxsize=None)
def _held(R, frame, far, s, bits):
    """check() of scene s's record (its bytes are the key: a 3-D batch that gives the planar bits is checked once)."""
    rm, pr, qr = _settings(len(SIZES))
    rec = np.frombuffer(bits, np.float32).reshape(SIZES[s], 2 * R)
    return T.check(rec, _pack(far), s, ray_directions(default_angles(R)), rm[s], pr[s], qr[s], frame=frame, mask=_masks()[s])


def _assert_inside(res, what):
    assert not res["bad"], f"{what}: {len(res['bad'])} rays outside the envelope, first: {res['bad'][0]}"
    assert res["ratio"] <= 1.0


# ---- 1. the device inside the envelope ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
@pytest.mark.parametrize("far", [False, True], ids=["origin", "shifted"])
@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("R", [1, 33, 64])
def test_device_lies_inside_the_float64_envelope(R, frame, far, z3):
    got = _device(R, frame, far, z3)
    worst, rays, wide, kinds = 0.0, 0, 0, set()
    for s, n in enumerate(SIZES):
        assert got[s].shape == (n, 2 * R)
        res = _held(R, frame, far, s, got[s].tobytes())
        _assert_inside(res, f"scene {s} (N = {n}), R = {R}, frame {frame}")
        assert res["rays"] == int(_masks()[s].sum()) * R
        worst, rays, wide, kinds = max(worst, res["ratio"]), rays + res["rays"], wide + res["wide"], kinds | res["kinds"]
    print(f"R = {R}, frame {frame}, {'shifted' if far else 'origin'}, {'3-D' if z3 else 'planar'}: {rays} rays, {wide} wide, "
          f"worst error / allowance of the device {worst:.3f}")
    assert wide <= 0.01 * rays + 1
    if R > 1:
        assert kinds == {0, 1, 2, 3, 4} and worst >= 0.05


@pytest.mark.parametrize("frame", [0, 1])
def test_translation_by_a_representable_shift_is_exact_on_the_device(frame):
    near = [T.quantised(G._scene(n, 7200 + q, dynamic=3)) for q, n in enumerate((65, 257))]
    far = [T.shifted(sc) for sc in near]
    a = SG._scanned(near, 20.0, 0.3, 0.1, R=33, frame=frame)
    b = SG._scanned(far, 20.0, 0.3, 0.1, R=33, frame=frame)
    for s in range(2):
        assert (a[s][:, 33:] > 0).any()
        SG._same(b[s], a[s], f"scene {s} shifted by {T.SHIFT}, frame {frame}")
        SG._same(a[s], scan_scene(near[s], default_angles(33), 20.0, 0.3, 0.1, frame=frame), f"scene {s}, frame {frame}")


# ---- 2. regimes the device has not seen -----------------------------------------------------------------------------------------

def _line(rng, start, count, step=0.1):
    a = rng.uniform(0, 2 * np.pi)
    return np.asarray(start) + step * np.arange(count)[:, None] * np.array([np.cos(a), np.sin(a)])


def _circle(centre, radius, count):
    a = 2 * np.pi * np.arange(count) / count
    return np.asarray(centre) + radius * np.column_stack([np.cos(a), np.sin(a)])


@lru_cache(maxsize=None)
def _sparse():
    """120 rows over 600 m x 600 m, three borders of 15 m, a ring of 2 m radius and a vehicle-sized ring, points 0.1 m apart."""
    rng = np.random.default_rng(31)
    loc = rng.uniform(-300, 300, (120, 2))
    return T.bare(loc, vel=rng.normal(0, 1, (120, 2)), wp=rng.uniform(-300, 300, (120, 2)),
                  borders=[_line(rng, rng.uniform(-250, 250, 2), 150) for _ in range(3)],
                  statics=[_circle(rng.uniform(-200, 200, 2), 2.0, 126)], vehicles=[_circle(rng.uniform(-200, 200, 2), 1.0, 60)])


@lru_cache(maxsize=None)
def _crowd(n=65):
    return G._scene(n, 7300 + n, dynamic=3)


def _ring_of_small_discs():
    a = default_angles(33)
    off = np.tile([0.0, 4e-4, -7e-4, 1.5e-3], 9)[:33]
    pts = 2.0 * np.column_stack([np.cos(a), np.sin(a)]) + off[:, None] * np.column_stack([-np.sin(a), np.cos(a)])
    return T.bare(np.vstack([[0, 0], pts])), np.abs(off) < 1e-3


def _regime(scenes, rm, pr, qr, dirs=None, R=33, frames=(0, 1), masks=None, envelope=True):
    """Device == twin bitwise, and (unit directions) the device inside the envelope.  Returns the frame-0 records and results."""
    B = len(scenes)
    rm, pr, qr = (list(np.broadcast_to(v, (B,))) for v in (rm, pr, qr))
    pk = pack_scenes(scenes)
    units = ray_directions(default_angles(R)) if dirs is None else dirs
    kw = dict(R=R) if dirs is None else dict(directions=dirs)
    out = {}
    for frame in frames:
        got = SG._scanned(scenes, rm, pr, qr, frame=frame, mask=masks, **kw)
        held = []
        for s, sc in enumerate(scenes):
            m = None if masks is None else pk_mask(masks[s], len(sc["loc"]))
            want = scan_scene(sc, None, rm[s], pr[s], qr[s], frame=frame, directions=units, mask=m)
            SG._same(got[s], want, f"scene {s}, frame {frame}")
            if envelope:
                res = T.check(got[s], pk, s, units, rm[s], pr[s], qr[s], frame=frame, mask=m)
                _assert_inside(res, f"scene {s}, frame {frame}")
                held.append(res)
        out[frame] = (got, held)
    return out


def pk_mask(m, n):
    out = np.zeros(n, bool)
    out[np.asarray(m)] = True
    return out


@pytest.mark.parametrize("Rmax", [250.0, 1000.0])
def test_long_ranges_over_a_sparse_scene(Rmax):
    out = _regime([_sparse(), _crowd(17)], Rmax, 0.5, 0.1)
    got, held = out[0]
    kinds = got[0][:, 33:]
    assert (kinds == 0).any() and all((kinds == k).any() for k in (1, 2, 3, 4))
    assert (got[0][:, :33][kinds > 0] > 100.0).any()                    # hits beyond anything the device had been run at
    print(f"Rmax = {Rmax:g}: {held[0]['wide']} of {held[0]['rays']} rays wide, worst error / allowance {held[0]['ratio']:.3f}")
    assert held[0]["wide"] <= 0.02 * held[0]["rays"]


def test_radius_of_a_millimetre():
    ring, inside = _ring_of_small_discs()
    out = _regime([ring, _crowd()], 20.0, 1e-3, 0.1, frames=(0,))
    got, held = out[0]
    assert np.array_equal(got[0][0, 33:] == 1, inside) and inside.sum() >= 24 and held[0]["wide"] == 0


def test_radius_larger_than_the_spacing():
    out = _regime([_crowd(), _crowd(129)], 20.0, 25.0, [0.1, 25.0])
    for s in range(2):
        got = out[0][0][s]
        assert (got[:, :33] == 0).mean() > 0.9 and (got[:, 33:] == 1).mean() > 0.9


def test_one_kind_switched_off_at_a_time():
    out = _regime([_crowd(), _crowd()], 20.0, [0.0, 0.3], [0.1, 0.0])
    got = out[0][0]
    assert not (got[0][:, 33:] == 1).any() and all((got[0][:, 33:] == k).any() for k in (2, 3, 4))
    assert set(np.unique(got[1][:, 33:])) <= {0.0, 1.0} and (got[1][:, 33:] == 1).any()


@pytest.mark.parametrize("length", [0.5, 2.0])
def test_directions_that_are_not_unit_vectors_follow_the_rules(length):
    """Defined by the rules only (include/sfm_hip.h): no geometric meaning is claimed, the device is the twin bit for bit."""
    ux, uy = ray_directions(default_angles(33))
    dirs = (np.float32(length) * ux, np.float32(length) * uy)
    out = _regime([_crowd(), _crowd(17)], [20.0, 6.0], 0.3, 0.1, dirs=dirs, envelope=False)
    unit = SG._scanned([_crowd()], 20.0, 0.3, 0.1, R=33)[0]
    assert (out[0][0][0] != unit).any()


def test_the_zero_direction():
    """(0, 0) passes set_scan's finiteness check.  By the rules t = c = 0, q = r2, w = r: every enabled disc is a candidate at
    range 0 and the first in the fixed order wins -- with many items, and with one agent row whose candidates four waves share."""
    ux, uy = (np.array(v) for v in ray_directions(default_angles(8)))
    ux[3] = uy[3] = 0.0
    alone = T.bare([[0.0, 0.0]])
    scenes = [_crowd(), _crowd(), _crowd(), alone, _crowd(257)]
    masks = [np.arange(65), [7], np.arange(65), [0], [100]]
    out = _regime(scenes, 20.0, [0.3, 0.3, 0.0, 0.3, 0.3], [0.1, 0.1, 0.1, 0.1, 0.0], dirs=(ux, uy), R=8, masks=masks, envelope=False)
    for frame in (0, 1):
        got = out[frame][0]
        for s, first in ((0, 1), (1, 1), (2, 2), (4, 1)):               # pedestrians first; without them the borders
            rows = pk_mask(masks[s], len(scenes[s]["loc"]))
            assert (got[s][rows, 3] == 0).all() and (got[s][rows, 8 + 3] == first).all(), (frame, s)
        assert got[3][0, 3] == 20.0 and got[3][0, 8 + 3] == 0            # nothing to see: a miss


def test_every_row_of_a_full_scene_at_one_ray():
    sc = G._scene(1024, 7400, dynamic=3)
    out = _regime([sc], 6.0, 0.3, 0.1, R=1)
    got, held = out[0]
    assert held[0]["rays"] == 1024 and len(set(np.unique(got[0][:, 1]))) >= 3


# ---- 3. item, share and tile boundaries, with a census --------------------------------------------------------------------------

def _cut(total, parts):
    """``total`` points as ``parts`` polylines of nearly equal length."""
    edges = np.linspace(0, total, parts + 1).astype(int)
    return [slice(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def _packed_scene(n, counts, seed, agent=None, winners=()):
    """n rows and counts = (borders, static, vehicle) points, uniformly over a disc of 6 m radius.  ``agent``: that row stands in
    the centre with nothing nearer than 1 m, except the geometry points ``winners``: point g of the run stands 0.5 m away exactly
    on ray q of 64, for (g, q) in winners."""
    rng = np.random.default_rng(seed)
    G_ = sum(counts)

    def disc(k, r0):
        r, a = np.sqrt(rng.uniform(r0 * r0, 36.0, k)), rng.uniform(0, 2 * np.pi, k)
        return np.column_stack([r * np.cos(a), r * np.sin(a)])

    loc, pts = disc(n, 1.0 if agent is not None else 0.0), disc(G_, 1.0 if agent is not None else 0.0)
    if agent is not None:
        loc[agent] = 0.0
        ux, uy = ray_directions(default_angles(64))
        for g, q in winners:
            pts[g] = 0.5 * np.float64([ux[q], uy[q]])
    nb, ns, nv = counts
    runs = [pts[:nb], pts[nb:nb + ns], pts[nb + ns:]]
    sc = T.bare(loc, vel=rng.normal(0, 1, (n, 2)), wp=disc(n, 0.0),
                borders=[runs[0][c] for c in _cut(nb, 3)], statics=[runs[1][c] for c in _cut(ns, 2)],
                vehicles=[runs[2][c] for c in _cut(nv, 2)])
    return sc


BIG = (600, 300, 200)                                                   # 1 100 points: three tiles, both kind boundaries in the second
EDGES = (0, 511, 512, 1023, 1024, 1099, 599, 600, 899, 900)            # first and last slot of every tile; either side of a kind boundary

# (rows, scanned rows, points per kind, R): n_scan R = 64, 65, 128, 129, 256, 257; G = 0, 1, 511, 512, 513, 1 100
CASES = {1: [(64, 64, (200, 200, 113), 1), (131, 65, BIG, 1), (128, 128, (200, 200, 111), 1), (129, 129, (200, 200, 112), 1),
             (300, 256, (0, 0, 1), 1), (257, 257, (0, 0, 0), 1)],
         64: [(41, 1, BIG, 64), (30, 2, (200, 200, 113), 64), (6, 4, (200, 200, 112), 64)],
         13: [(17, 5, (200, 200, 111), 13), (9, 5, (1, 0, 0), 13)],
         43: [(66, 3, BIG, 43)]}


@lru_cache(maxsize=None)
def _boundary_batch(R):
    scenes, masks = [], []
    for q, (n, n_scan, counts, _) in enumerate(CASES[R]):
        designed = R == 64 and q == 0
        scenes.append(_packed_scene(n, counts, 7500 + 10 * R + q, agent=0 if designed else None,
                                    winners=tuple((g, 5 * k + 2) for k, g in enumerate(EDGES)) if designed else ()))
        masks.append(np.arange(n_scan) if designed else np.round(np.linspace(0, n - 1, n_scan)).astype(int))
    return scenes, masks


def _split(items):
    return 4 if items <= ITEMS_4 else 2 if items <= ITEMS_2 else 1


def test_the_boundary_scenes_hold_what_they_were_built_for():
    """From the scenes and the float64 reference alone."""
    items, points, shares, tiles, slots = set(), set(), set(), set(), set()
    for R in CASES:
        scenes, masks = _boundary_batch(R)
        pk = pack_scenes(scenes)
        for s, (n, n_scan, counts, _) in enumerate(CASES[R]):
            st, geo = T.scene_arrays(pk, s)
            assert len(st["x"]) == n and tuple(len(g[0]) for g in geo) == counts and len(set(masks[s])) == n_scan
            nb, ns, nv = counts
            G_, T_ = nb + ns + nv, n + nb + ns + nv
            items.add(n_scan * R)
            points.add(G_)
            split = _split(n_scan * R)
            kind_edges = {n, n + nb, n + nb + ns}
            if G_ > TILE:                                               # the kind boundaries fall inside a tile, not on its edge
                assert nb % TILE and (nb + ns) % TILE and (counts != BIG or nb // TILE == (nb + ns) // TILE == 1)
            if split > 1 and G_ >= 511:                                 # a wave's share ends inside a kind, not between two
                cuts = {T_ * k // split for k in range(1, split)}
                assert not cuts & kind_edges and all(0 < c < T_ for c in cuts)
                assert any(c > n for c in cuts)                         # ... and inside the geometry at least once
            res = T.check(np.zeros((n, 2 * R), np.float32), pk, s, ray_directions(default_angles(R)), 8.0, 0.2, 0.1,
                          mask=pk_mask(masks[s], n))
            for v in res["first"].values():                             # where the nearest candidate, beyond doubt, sits in the walk
                if split > 1:
                    shares.add((split, next(k for k in range(split) if T_ * k // split <= v < T_ * (k + 1) // split)))
                if v >= n and G_ > TILE:
                    tiles.add((v - n) // TILE)
                    slots.add((v - n) if (R == 64 and s == 0) else None)
    assert items == {64, 65, 128, 129, 256, 257} and points >= {0, 1, 511, 512, 513} and max(points) >= 1025
    assert shares == {(4, 0), (4, 1), (4, 2), (4, 3), (2, 0), (2, 1)}, shares
    assert tiles == {0, 1, 2} and slots >= set(EDGES), (tiles, set(EDGES) - slots)


@pytest.mark.parametrize("R", sorted(CASES))
def test_item_share_and_tile_boundaries(R):
    scenes, masks = _boundary_batch(R)
    out = _regime(scenes, 8.0, 0.2, 0.1, R=R, masks=[list(m) for m in masks])
    for frame, (got, held) in out.items():
        for s, res in enumerate(held):
            assert res["rays"] == CASES[R][s][1] * R
    if R == 64:                                                         # the designed winners, as the device saw them
        got = out[0][0][0]
        for k, g in enumerate(EDGES):
            want = 2 if g < BIG[0] else 3 if g < BIG[0] + BIG[1] else 4
            assert got[0, 64 + 5 * k + 2] == want and abs(got[0, 5 * k + 2] - 0.4) < 1e-6, (g, got[0, 5 * k + 2], got[0, 64 + 5 * k + 2])
