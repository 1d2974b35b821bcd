"""Host-side tests of the batch's range scans (no GPU): the exact ``fmaf`` of the host twin against rational arithmetic, analytic
cases of ``scan.scan_scene`` with exactly representable values (include/sfm_hip.h, ABI 17), the rotation of the record with the
rays, the twin's exact pruning against the unpruned walk, the packers' refusals and the ABI 17 entries in header and binding."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd import batch as B_
from carla_social_force_model_amd.scan import (MAX_SCAN_RAYS, _fma32, check_directions, default_angles, radius2, ray_directions,
                                               scan_arrays, scan_mask, scan_scene)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = (np.float32([1, 0, -1, 0]), np.float32([0, 1, 0, -1]))


def _bare(loc, vel=None, wp=None, **more):
    loc = np.asarray(loc, dtype=np.float64).reshape(-1, 2)
    n = len(loc)
    z = np.zeros((n, 1))
    sc = {"loc": np.hstack([loc, z]),
          "vel": np.hstack([np.zeros((n, 2)) if vel is None else np.asarray(vel, dtype=np.float64).reshape(n, 2), z]),
          "waypoint": np.hstack([loc + 1.0 if wp is None else np.asarray(wp, dtype=np.float64).reshape(n, 2), z]),
          "target_speed": np.ones(n)}
    sc.update(more)
    return sc


# ---- the exact fmaf -------------------------------------------------------------------------------------------------------------

def _round32(fr):
    """A rational -> the nearest float32, ties to even (the values used here neither overflow nor need a NaN)."""
    if fr == 0:
        return np.float32(0.0)
    sign, m = (-1, -fr) if fr < 0 else (1, fr)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    k = m / quantum
    lo = k.numerator // k.denominator
    rest = k - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    return np.float32(sign * float(lo * quantum))


def _triples():
    rng = np.random.default_rng(17)
    out = []
    # exact fp32 midpoints: (1 + k 2^-12)(1 + m 2^-12) = 1 + (k + m) 2^-12 + k m 2^-24 with k m odd sits half way between two
    # float32; c = 0 keeps the tie, c = +-2^-e moves the sum off it by less than the float64 sum can hold
    for _ in range(600):
        k, m = (int(v) | 1 for v in rng.integers(1, 2 ** 11, 2))
        a, b = 1.0 + k * 2.0 ** -12, 1.0 + m * 2.0 ** -12
        for c in (0.0, 2.0 ** -int(rng.integers(40, 100)), -(2.0 ** -int(rng.integers(40, 100)))):
            out.append((a, b, c))
            out.append((-a, b, -c))
    # cancellation: c close to -a b, so the low bits of the product decide
    for _ in range(1000):
        a, b = np.float32(rng.normal(0, 3.0, 2))
        c = np.float32(-np.float64(a) * np.float64(b)) * np.float32(1.0 + rng.integers(-2, 3) * 2.0 ** -23)
        out.append((float(a), float(b), float(c)))
    # wide exponent spread, denormal results included
    for _ in range(1200):
        ea, eb, ec = rng.integers(-70, 40, 3)
        a, b, c = (np.float32(rng.uniform(1, 2) * 2.0 ** int(e) * rng.choice([-1, 1])) for e in (ea, eb, ec))
        out.append((float(a), float(b), float(c)))
    for _ in range(300):
        a = np.float32(rng.uniform(1, 2) * 2.0 ** -70)
        b = np.float32(rng.uniform(1, 2) * 2.0 ** -70)
        c = np.float32(rng.integers(-3, 4) * 2.0 ** -149)
        out.append((float(a), float(b), float(c)))
    return np.float32(out)


def test_fma32_matches_exact_rational_arithmetic():
    t = _triples()
    assert len(t) > 3000
    got = _fma32(t[:, 0], t[:, 1], t[:, 2])
    assert got.dtype == np.float32
    want = np.float32([_round32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))) for a, b, c in t])
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{bad.size} triples differ, first {t[bad[0]]}: {got[bad[0]]!r} against {want[bad[0]]!r}"
    # the float64 idiom without the repair is off by an ulp on some of them: the triples are adversarial
    naive = (t[:, 0].astype(np.float64) * t[:, 1].astype(np.float64) + t[:, 2].astype(np.float64)).astype(np.float32)
    assert (naive != want).any()


def test_fma32_passes_infinities_and_nans_through():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    with np.errstate(all="ignore"):
        got = _fma32(np.float32([inf, 1e30, nan, 2.0]), np.float32([2.0, 1e30, 1.0, 3.0]), np.float32([1.0, 1.0, 1.0, -inf]))
    assert got[0] == inf and got[1] == inf and np.isnan(got[2]) and got[3] == -inf


# ---- analytic cases -------------------------------------------------------------------------------------------------------------

def _scan1(sc, Rmax=10.0, ped=0.5, point=0.5, **kw):
    kw.setdefault("directions", AXES)
    return scan_scene(sc, None, Rmax, ped, point, **kw)


def test_a_disc_dead_ahead_and_the_same_disc_behind():
    rec = _scan1(_bare([[0, 0], [3, 0]]))
    assert rec.shape == (2, 8) and rec.dtype == np.float32
    assert np.array_equal(rec[0], np.float32([2.5, 10, 10, 10, 1, 0, 0, 0]))          # ahead on ray 0: 3 - 0.5
    assert np.array_equal(rec[1], np.float32([10, 10, 2.5, 10, 0, 0, 1, 0]))          # row 1 sees row 0 on ray 2, nothing on ray 0


def test_inside_a_disc_the_range_is_zero():
    rec = _scan1(_bare([[0, 0], [0.25, 0]]))
    assert np.array_equal(rec[0, :4], np.float32([0, 0, 0, 0])) and np.array_equal(rec[0, 4:], np.float32([1, 1, 1, 1]))
    assert np.signbit(rec[0, :4]).sum() == 0


def test_order_rule_and_every_kind():
    border = [np.array([[3.0, 0.0]])]
    rec = _scan1(_bare([[0, 0], [3, 0]], borders=border))
    assert rec[0, 0] == 2.5 and rec[0, 4] == 1                                        # pedestrian and border disc at the same range
    rec = _scan1(_bare([[0, 0], [4, 0]], borders=border))
    assert rec[0, 0] == 2.5 and rec[0, 4] == 2                                        # the border disc is nearer
    c = np.zeros(2)
    sc = _bare([[0, 0]], borders=[np.array([[0.0, 2.0]])], static_obstacles=[(c, np.array([[-3.0, 0.0]]))],
               dynamic_obstacles=[(c, np.array([[0.0, -4.0], [np.inf, np.inf]]))])
    rec = _scan1(sc)
    assert np.array_equal(rec[0], np.float32([10, 1.5, 2.5, 3.5, 0, 2, 3, 4]))
    two = _bare([[0, 0]], borders=[np.array([[5.0, 0.0]]), np.array([[3.0, 0.0], [3.0, 0.0]])])
    assert _scan1(two)[0, 0] == 2.5


def test_a_range_equal_to_max_range_is_a_miss():
    sc = _bare([[0, 0], [3, 0]])
    assert np.array_equal(_scan1(sc, Rmax=2.5)[0, [0, 4]], np.float32([2.5, 0]))       # s == Rmax: strict `<`
    assert np.array_equal(_scan1(sc, Rmax=2.75)[0, [0, 4]], np.float32([2.5, 1]))
    assert np.array_equal(_scan1(sc, Rmax=2.0)[0, [0, 4]], np.float32([2.0, 0]))


def test_radius_zero_switches_a_kind_off():
    sc = _bare([[0, 0], [3, 0]], borders=[np.array([[0.0, 3.0]])])
    rec = _scan1(sc, ped=0.0)
    assert np.array_equal(rec[0], np.float32([10, 2.5, 10, 10, 0, 2, 0, 0]))
    rec = _scan1(sc, point=0.0)
    assert np.array_equal(rec[0], np.float32([2.5, 10, 10, 10, 1, 0, 0, 0]))


def test_ghost_rows_and_nan_rows_are_zero_and_unseen():
    sc = _bare([[0, 0], [3.0e15, 0], [np.nan, 0], [0, np.nan], [3, 0]])
    rec = _scan1(sc)
    assert not rec[1:4].any()
    assert np.array_equal(rec[0], np.float32([2.5, 10, 10, 10, 1, 0, 0, 0]))
    assert np.array_equal(rec[4], np.float32([10, 10, 2.5, 10, 0, 0, 1, 0]))
    assert np.array_equal(_scan1(sc, prune=False), rec)


def test_mask_and_state_and_3d():
    sc = _bare([[0, 0], [3, 0], [0, 3]])
    rec = _scan1(sc, mask=[True, False, True])
    assert not rec[1].any() and rec[0, 0] == 2.5 and rec[0, 1] == 2.5 and rec[2, 3] == 2.5
    moved = (np.array([[0.0, 0, 7], [2, 0, 7], [0, 3, 7]]), np.zeros((3, 3)))
    assert _scan1(sc, state=moved)[0, 0] == 1.5


def test_heading_frame():
    # v = (0, 2): the heading is (0, 1), so ray 0 looks along +y
    sc = _bare([[0, 0], [0, 3], [3, 0]], vel=[[0, 2], [0, 0], [0, 0]], wp=[[5, 5], [0, 3], [3, -4]])
    rec = _scan1(sc, frame=1)
    assert np.array_equal(rec[0], np.float32([2.5, 10, 10, 2.5, 1, 0, 0, 1]))          # ray 3 = heading rotated by -90 degrees: +x
    assert np.array_equal(rec[1], _scan1(sc)[1])                                       # no speed, at its goal: (1, 0), frame 0
    assert np.array_equal(rec[2], np.float32([10, 10, 10, 2.5, 0, 0, 0, 1]))           # goal straight down: row 0 is to its right
    sc["waypoint"][2, :2] = [-1.0, 0.0]                                                # the goal's direction is (-1, 0)
    assert np.array_equal(_scan1(sc, frame=1)[2], np.float32([2.5, 10, 10, 10, 1, 0, 0, 0]))


def test_rotating_the_rays_rotates_the_record():
    sc = vars(scenarios.make_scenario(40, 5, n_borders=6, n_static=3, n_dynamic=2, border_len=(3.0, 15.0)))
    rec = scan_scene(sc, None, 6.0, 0.3, 0.1, directions=AXES)
    assert (rec[:, 4:] > 0).any() and (rec[:, 4:] == 0).any()
    turned = scan_scene(sc, None, 6.0, 0.3, 0.1, directions=(np.roll(AXES[0], -1), np.roll(AXES[1], -1)))
    assert np.array_equal(turned[:, :4], np.roll(rec[:, :4], -1, axis=1)) and np.array_equal(turned[:, 4:], np.roll(rec[:, 4:], -1, axis=1))


@pytest.mark.parametrize("frame", [0, 1])
def test_pruning_changes_nothing(frame):
    for q, (n, Rmax, pr, qr) in enumerate(((30, 3.0, 0.3, 0.1), (64, 1.0, 0.45, 0.25), (17, 8.0, 0.2, 0.0), (5, 0.05, 0.3, 0.1))):
        sc = vars(scenarios.make_scenario(n, 60 + q, n_borders=6, n_static=3, n_dynamic=2, border_len=(3.0, 15.0)))
        a = scan_scene(sc, default_angles(16), Rmax, pr, qr, frame=frame)
        b = scan_scene(sc, default_angles(16), Rmax, pr, qr, frame=frame, prune=False)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (n, Rmax)
        assert (a[:, :16] < np.float32(Rmax)).any() or Rmax < 0.1


# ---- packers --------------------------------------------------------------------------------------------------------------------

def test_ray_directions():
    dx, dy = ray_directions(default_angles(8))
    assert dx.dtype == np.float32 and dx.shape == (8,) and dx[0] == 1 and dy[0] == 0
    assert np.array_equal(dx, np.cos(2 * np.pi * np.arange(8) / 8).astype(np.float32))
    assert np.array_equal(dy, np.sin(2 * np.pi * np.arange(8) / 8).astype(np.float32))
    for bad in ([], np.zeros(MAX_SCAN_RAYS + 1), np.zeros((2, 2)), 1.0):
        with pytest.raises(ValueError, match="angles: expected"):
            ray_directions(bad)
    for bad in ([0.0, np.nan], [np.inf]):
        with pytest.raises(ValueError, match="finite"):
            ray_directions(bad)
    with pytest.raises(ValueError, match="numbers"):
        ray_directions(["east"])
    for bad in (0, MAX_SCAN_RAYS + 1):
        with pytest.raises(ValueError, match="R must be"):
            default_angles(bad)
    with pytest.raises(ValueError, match="finite"):
        check_directions(([1.0, np.nan], [0.0, 1.0]))
    with pytest.raises(ValueError, match="finite"):
        check_directions(([1.0e39], [0.0]))
    with pytest.raises(ValueError, match="directions"):
        check_directions(([1.0, 0.0], [0.0]))
    with pytest.raises(ValueError, match="pair"):
        check_directions(5)


def test_scan_arrays_and_their_refusals():
    rm, rp, rq, frame = scan_arrays(3, 4.0, [0.3, 0.0, 0.5], frame=1)
    assert all(a.dtype == np.float32 and a.shape == (3,) for a in (rm, rp, rq)) and frame == 1
    assert np.array_equal(rm, np.float32([4, 4, 4])) and np.array_equal(rp, np.float32([0.3, 0.0, 0.5]))
    assert np.array_equal(rq, np.float32([0.1, 0.1, 0.1]))
    for bad in (np.nan, 0.0, -1.0, np.inf, 2.0e6):
        with pytest.raises(ValueError, match="max_range must be finite, > 0"):
            scan_arrays(3, [4.0, bad, 4.0], 0.3)
    for bad in (np.nan, -0.5, np.inf, 2.0e6):
        with pytest.raises(ValueError, match="ped_radius must be finite, >= 0"):
            scan_arrays(3, 4.0, bad)
        with pytest.raises(ValueError, match="point_radius must be finite, >= 0"):
            scan_arrays(3, 4.0, 0.3, [0.1, 0.1, bad])
    for bad in (2, -1, True, 0.0):
        with pytest.raises(ValueError, match="frame must be"):
            scan_arrays(3, 4.0, 0.3, frame=bad)
    with pytest.raises(ValueError, match="max_range: expected a scalar or 3 values"):
        scan_arrays(3, [4.0, 4.0], 0.3)
    with pytest.raises(ValueError, match="ped_radius must be numbers"):
        scan_arrays(3, 4.0, "wide")
    assert radius2(0.1) == np.float32(np.float64(np.float32(0.1)) ** 2)


def test_scan_mask():
    so = np.array([0, 3, 3, 5], np.int32)
    assert scan_mask(None, so) is None
    assert np.array_equal(scan_mask([[0, 2], [], True], so), np.uint8([1, 0, 1, 1, 1]))
    assert np.array_equal(scan_mask([np.array([False, True, False]), False, np.array([1])], so), np.uint8([0, 1, 0, 0, 1]))
    assert np.array_equal(scan_mask(np.array([True, False, False, False, True]), so), np.uint8([1, 0, 0, 0, 1]))
    with pytest.raises(ValueError, match="3 scenes"):
        scan_mask([[0]], so)
    with pytest.raises(ValueError, match="row indices must lie"):
        scan_mask([[3], [], []], so)
    with pytest.raises(ValueError, match="bool mask of shape"):
        scan_mask([np.array([True]), [], []], so)
    with pytest.raises(ValueError, match="concatenated rows"):
        scan_mask(np.ones(4, bool), so)
    with pytest.raises(ValueError, match="concatenated rows"):
        scan_mask(np.ones(5), so)


def test_twin_refuses_bad_settings():
    sc = _bare([[0, 0]])
    with pytest.raises(ValueError, match="frame"):
        scan_scene(sc, [0.0], 4.0, 0.3, 0.1, frame=2)
    with pytest.raises(ValueError, match="max_range"):
        scan_scene(sc, [0.0], 0.0, 0.3, 0.1)
    with pytest.raises(ValueError, match="ped_radius"):
        scan_scene(sc, [0.0], 4.0, -0.3, 0.1)
    assert scan_scene(_bare(np.zeros((0, 2))), [0.0, 1.0], 4.0, 0.3, 0.1).shape == (0, 4)


def test_abi17_entry_points_are_declared():
    assert _lib.ABI_VERSION >= 17
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert int(re.search(r"#define SFM_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    names = ("sfm_batch_set_scan", "sfm_batch_scan", "sfm_batch_download_scan")
    for name in names:
        assert name in _lib.SYMBOLS and _lib.SINCE[name] == 17
        assert re.search(r"^int " + name + r"\(SfmBatch\* b", header, re.M), name
    assert [len(_lib.SYMBOLS[n][1]) for n in names] == [9, 1, 2]
    for name, val in (("SFM_BATCH_PTR_SCAN", B_.PTR_SCAN), ("SFM_BATCH_MAX_SCAN_RAYS", MAX_SCAN_RAYS)):
        assert re.search(r"#define " + name + r" " + str(val) + r"\b", header), name
    lib = _lib.load()                                                   # bound: the built library exports them
    for name in names:
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
    assert lib.sfm_abi_version() == 17


def test_lidar_loop_example_imports_and_its_policy_reads_the_scan():
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("batch_lidar_loop", os.path.join(ROOT, "examples", "batch_lidar_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    dirs = torch.as_tensor(np.stack(ray_directions(default_angles(4)), axis=1))
    goal, speed = torch.tensor([[3.0, 0.0], [0.0, -2.0]]), torch.tensor([[1.0], [1.5]])
    free = torch.full((2, 4), 5.0)
    v = ex.policy(goal, speed, free, dirs)
    assert torch.allclose(v, torch.tensor([[1.0, 0.0], [0.0, -1.5]]), atol=1e-6)      # nothing near: towards the goal at the target speed
    near = free.clone()
    near[0, 0] = 0.5                                                                   # something 0.5 m ahead of agent 0: pushed back
    assert ex.policy(goal, speed, near, dirs)[0, 0] < v[0, 0] and torch.equal(ex.policy(goal, speed, near, dirs)[1], v[1])
