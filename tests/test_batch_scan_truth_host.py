"""Host-side tests (no GPU) that say what the range scan's record MEANS: the host twin ``scan.scan_scene`` against a float64 ray cast
written from the geometry (``_scan_truth``), inside an interval derived operation by operation from the rules of include/sfm_hip.h.
Generated crowds in both frames, at the origin and far from it; designed grazes, boundaries, near ties and range limits, each with
the interval as wide or as narrow as it was designed; frame 1 at generic headings; exact translation; and copies of the twin with
one line changed, which the tests of this module must refuse."""
import inspect
from functools import lru_cache

import numpy as np
import pytest

import _scan_truth as T
import test_batch_scan_host as H
from carla_social_force_model_amd import scan as S
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd.batch import pack_scenes
from carla_social_force_model_amd.scan import default_angles, ray_directions, scan_scene

SIZES = (17, 65, 300)
RMAX, PED, POINT = 20.0, 0.3, 0.1
PLUS_X = (np.float32([1.0]), np.float32([0.0]))


def _step(v, k):
    """The float32 k steps above (k > 0) or below v."""
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


@lru_cache(maxsize=None)
def _crowd(n, far):
    sc = vars(scenarios.make_scenario(n, 7000 + n, n_borders=6, n_static=3, n_dynamic=3, border_len=(3.0, 15.0)))
    return T.shifted(sc) if far else sc


@lru_cache(maxsize=None)
def _checked_crowd(n, R, frame, far, twin=scan_scene):
    sc = _crowd(n, far)
    rec = twin(sc, default_angles(R), RMAX, PED, POINT, frame=frame)
    return T.check(rec, pack_scenes([sc]), 0, ray_directions(default_angles(R)), RMAX, PED, POINT, frame=frame)


def _check(sc, dirs, Rmax, ped, point, frame=0, rec=None, twin=scan_scene):
    """The twin's record of a designed scene (or ``rec``) held to the interval: (record, check's result)."""
    if rec is None:
        rec = twin(sc, None, Rmax, ped, point, frame=frame, directions=dirs)
    return rec, T.check(rec, pack_scenes([sc]), 0, dirs, Rmax, ped, point, frame=frame)


def _with(rec, rng, kind):
    """``rec`` with row 0's single ray replaced."""
    out = np.array(rec, dtype=np.float32)
    out[0] = [rng, kind]
    return out


def _row0(sc, dirs, Rmax, ped, point, frame=0):
    return dict(T.cast(pack_scenes([sc]), 0, dirs, Rmax, ped, point, frame))[0]


# ---- 1. the twin inside the envelope, generated crowds --------------------------------------------------------------------------

@pytest.mark.parametrize("far", [False, True], ids=["origin", "shifted"])
@pytest.mark.parametrize("frame", [0, 1])
@pytest.mark.parametrize("R", [33, 64])
@pytest.mark.parametrize("n", SIZES)
def test_twin_lies_inside_the_float64_envelope(n, R, frame, far):
    res = _checked_crowd(n, R, frame, far)
    print(f"N = {n}, R = {R}, frame {frame}, {'shifted' if far else 'origin'}: {res['rays']} rays, {res['wide']} wide, "
          f"worst error / allowance {res['ratio']:.3f} at {res['at']}")
    assert res["rays"] == n * R
    assert not res["bad"], f"{len(res['bad'])} rays outside, first: {res['bad'][0]}"
    assert res["ratio"] <= 1.0


def test_the_envelope_is_not_vacuous():
    """A condition on the reference alone: on these crowds the interval is narrow on all but 1 % of the rays, every kind and the
    miss occur among the narrow ones, and the allowance is neither exceeded nor idle."""
    worst = 0.0
    for n in SIZES:
        for R in (33, 64):
            for frame in (0, 1):
                for far in (False, True):
                    res = _checked_crowd(n, R, frame, far)
                    assert res["wide"] <= 0.01 * res["rays"], (n, R, frame, far, res["wide"], res["rays"])
                    assert res["kinds"] == {0, 1, 2, 3, 4}, (n, R, frame, far, res["kinds"])
                    assert len(res["first"]) > 0.5 * res["rays"]       # most rays have a nearest candidate beyond doubt
                    worst = max(worst, res["ratio"])
    print(f"worst error / allowance of the twin over all crowds: {worst:.3f}")
    assert 0.05 <= worst <= 1.0


# ---- 2. designed hard cases -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [-64, -1, 0, 1, 64])
def test_a_graze_within_a_few_ulp(k):
    """A disc of radius 0.5 whose centre is 0.5 off the +x ray, k float32 steps further out (k < 0: further in), and a second
    disc dead ahead at 8.  Within a step the rules may go either way: anything from the graze at 3 to the disc behind it at 7.5.
    64 steps inside it is a hit with a narrow interval, 64 steps outside it cannot be one."""
    sc = T.bare([[0, 0], [3, _step(0.5, k)], [8, 0]])
    rec, res = _check(sc, PLUS_X, 20.0, 0.5, 0.0)
    assert not res["bad"], res["bad"]
    o = _row0(sc, PLUS_X, 20.0, 0.5, 0.0)
    graze = int(np.flatnonzero(o.order == 1)[0])
    if abs(k) <= 1:
        assert o.possible[0, graze] and not o.certain[0, graze]
        assert 2.99 < o.lo[0] < 3.0 and 7.5 < o.hi[0] < 7.50001
    elif k < 0:
        assert o.certain[0, graze] and 2.99 < o.lo[0] < o.hi[0] < 3.0 and o.hi[0] - o.lo[0] < 1e-3
        assert rec[0, 1] == 1 and 2.99 < rec[0, 0] < 3.0
    else:
        assert not o.possible[0, graze] and 7.49999 < o.lo[0] <= 7.5 <= o.hi[0] < 7.50001
        assert rec[0, 1] == 1 and rec[0, 0] == 7.5


@pytest.mark.parametrize("angle", [0.0, 0.7, 2.9])
@pytest.mark.parametrize("k", [-3, -1, 0, 1, 3])
def test_an_origin_a_few_ulp_from_the_boundary(k, angle):
    """The disc's centre lies 0.5 (k steps more, or fewer) along the ray and its radius is 0.5: the origin is on the boundary, a few
    ulp outside or inside.  t - w does not cancel badly here (w is r, to rounding): the interval stays below a micrometre."""
    dirs = ray_directions([angle])
    far = np.float64(_step(0.5, k))
    sc = T.bare([[0, 0], [far * np.float64(dirs[0][0]), far * np.float64(dirs[1][0])]])
    rec, res = _check(sc, dirs, 20.0, 0.5, 0.0)
    assert not res["bad"], res["bad"]
    o = _row0(sc, dirs, 20.0, 0.5, 0.0)
    assert o.certain[0, 0] and o.lo[0] < 2e-7 and o.hi[0] < 1e-6 and (k < 3 or o.lo[0] > 0)
    assert rec[0, 1] == 1 and 0.0 <= rec[0, 0] < 1e-6
    if angle == 0.0:
        assert rec[0, 0] == max(np.float32(far) - np.float32(0.5), 0)  # exact on the axis (Sterbenz)


def test_a_disc_centred_behind_that_still_covers_the_origin():
    sc = T.bare([[0, 0], [-0.3, 0.1]])
    rec, res = _check(sc, PLUS_X, 20.0, 0.5, 0.0)
    o = _row0(sc, PLUS_X, 20.0, 0.5, 0.0)
    assert not res["bad"] and o.certain[0, 0] and o.lo[0] == 0.0 and o.hi[0] < 1e-6
    assert rec[0, 0] == 0.0 and rec[0, 1] == 1
    sc = T.bare([[0, 0], [-3.0, 0.1]])                                   # wholly behind: no hit, and the interval is a point
    rec, res = _check(sc, PLUS_X, 20.0, 0.5, 0.0)
    o = _row0(sc, PLUS_X, 20.0, 0.5, 0.0)
    assert not res["bad"] and not o.possible.any() and rec[0, 0] == 20.0 and rec[0, 1] == 0
    for wrong in ([2.5, 1], [0.0, 1], [20.0, 1], [19.0, 0]):
        assert _check(sc, PLUS_X, 20.0, 0.5, 0.0, rec=_with(rec, *wrong))[1]["bad"], wrong


def test_two_kinds_closer_than_and_further_than_their_allowances():
    """A pedestrian disc at range 2.5 and a border disc one float32 step behind it (2.4e-7, inside the allowance of about 5e-7 on
    either): the interval admits both kinds.  With the border disc a millimetre behind, only the pedestrian."""
    near = T.bare([[0, 0], [3, 0]], borders=[[[_step(2.6, 1), 0]]])
    rec, res = _check(near, PLUS_X, 20.0, 0.5, 0.1)
    assert not res["bad"] and rec[0, 1] == 1
    o = _row0(near, PLUS_X, 20.0, 0.5, 0.1)
    assert o.certain.all() and o.lo_k[0].max() < o.hi_k[0].min() and 1e-7 < o.hi[0] - o.lo[0] < 2e-6
    assert not _check(near, PLUS_X, 20.0, 0.5, 0.1, rec=_with(rec, _step(2.5, 1), 2))[1]["bad"]
    apart = T.bare([[0, 0], [3, 0]], borders=[[[2.601, 0]]])
    rec, res = _check(apart, PLUS_X, 20.0, 0.5, 0.1)
    assert not res["bad"] and rec[0, 1] == 1 and res["first"] == {(0, 0): 1}
    o = _row0(apart, PLUS_X, 20.0, 0.5, 0.1)
    assert o.hi_k[0].min() < o.lo_k[0].max() and o.hi[0] - o.lo[0] < 2e-6
    for wrong in ([2.5, 2], [2.501, 2], [2.501, 1], [2.50001, 1]):
        assert _check(apart, PLUS_X, 20.0, 0.5, 0.1, rec=_with(rec, *wrong))[1]["bad"], wrong


def test_a_candidate_within_an_allowance_of_the_range_limit():
    """A disc at range 2.5 with Rmax two steps below, at, and two steps above 2.5 (within the allowance: a hit and a miss are both
    inside), and a millimetre either side (only one of them is)."""
    sc = T.bare([[0, 0], [3, 0]])
    for k in (-2, 0, 2):
        Rmax = _step(2.5, k)
        rec, res = _check(sc, PLUS_X, Rmax, 0.5, 0.0)
        assert not res["bad"], (k, res["bad"])
        assert (rec[0, 1] == 1) == (k > 0)
        o = _row0(sc, PLUS_X, Rmax, 0.5, 0.0)
        assert o.lo[0] < Rmax and o.hi[0] > Rmax
        assert not _check(sc, PLUS_X, Rmax, 0.5, 0.0, rec=_with(rec, Rmax, 0))[1]["bad"]          # the miss is inside
        if k > 0:
            assert not _check(sc, PLUS_X, Rmax, 0.5, 0.0, rec=_with(rec, 2.5, 1))[1]["bad"]
    rec, res = _check(sc, PLUS_X, 2.501, 0.5, 0.0)
    assert not res["bad"] and rec[0, 1] == 1
    assert _check(sc, PLUS_X, 2.501, 0.5, 0.0, rec=_with(rec, 2.501, 0))[1]["bad"]                    # a millimetre inside: a hit
    rec, res = _check(sc, PLUS_X, 2.499, 0.5, 0.0)
    assert not res["bad"] and rec[0, 1] == 0
    assert _check(sc, PLUS_X, 2.499, 0.5, 0.0, rec=_with(rec, 2.49, 1))[1]["bad"]                     # a millimetre outside: a miss


def test_a_disc_300_m_away_at_a_range_limit_of_1000():
    dirs = ray_directions([0.7])
    u = np.float64([np.cos(0.7), np.sin(0.7)])
    sc = T.bare([[0, 0], 300.0 * u + 0.2 * np.float64([-u[1], u[0]])])
    rec, res = _check(sc, dirs, 1000.0, 0.5, 0.0)
    assert not res["bad"], res["bad"]
    o = _row0(sc, dirs, 1000.0, 0.5, 0.0)
    assert rec[0, 1] == 1 and 299.5 < rec[0, 0] < 299.6 and o.certain.all()
    assert 2e-5 < o.hi[0] - o.lo[0] < 1e-3                              # about 2^-24 (4 d + 4 d |c| / w) either side
    assert res["wide"] == 0 and 0.0 < res["ratio"] <= 1.0


def _ring_of_small_discs():
    a = default_angles(33)
    off = np.tile([0.0, 4e-4, -7e-4, 1.5e-3], 9)[:33]                  # across the ray: inside the millimetre three times in four
    pts = 2.0 * np.column_stack([np.cos(a), np.sin(a)]) + off[:, None] * np.column_stack([-np.sin(a), np.cos(a)])
    return T.bare(np.vstack([[0, 0], pts])), off


def test_radius_of_a_millimetre():
    sc, off = _ring_of_small_discs()
    dirs = ray_directions(default_angles(33))
    rec, res = _check(sc, dirs, 20.0, 1e-3, 0.0)
    assert not res["bad"], res["bad"]
    assert np.array_equal(rec[0, 33:] == 1, np.abs(off) < 1e-3) and res["wide"] == 0
    assert (np.abs(rec[0, :33][np.abs(off) < 1e-3] - 2.0) < 1.1e-3).all()
    thick = scan_scene(sc, None, 20.0, 1.1e-3, 0.0, directions=dirs)     # a radius a tenth larger is outside
    assert T.check(thick, pack_scenes([sc]), 0, dirs, 20.0, 1e-3, 0.0)["bad"]


def test_radius_larger_than_the_spacing():
    sc = _crowd(65, False)
    dirs = ray_directions(default_angles(33))
    rec, res = _check(sc, dirs, 20.0, 25.0, 0.1)
    assert not res["bad"], res["bad"][:1]
    assert (rec[:, :33] == 0).mean() > 0.9 and (rec[:, 33:] == 1).mean() > 0.9 and res["wide"] <= 0.01 * res["rays"]


# ---- 3. frame 1 at generic headings ---------------------------------------------------------------------------------------------

def test_frame_1_at_generic_headings():
    sc = dict(_crowd(65, False))
    vel, wp = np.array(sc["vel"]), np.array(sc["waypoint"])
    vel[::3] = 0.0                                                      # at rest: the goal entry
    vel[6] = 0.0
    wp[6] = sc["loc"][6]                                                # neither: (1, 0)
    sc["vel"], sc["waypoint"] = vel, wp
    pk = pack_scenes([sc])
    st, _ = T.scene_arrays(pk, 0)
    heads = [T.heading64(st, i) for i in range(65)]
    assert {h[2] for h in heads} == {"v", "goal", "none"} and heads[6][2] == "none"
    assert sum(h[2] == "goal" for h in heads) >= 20 and sum(h[2] == "v" for h in heads) >= 40
    assert all(min(abs(h[0]), abs(h[1])) > 0.01 for h in heads if h[2] != "none")     # none of them along an axis
    dirs = ray_directions(default_angles(33))
    rec, res = _check(sc, dirs, RMAX, PED, POINT, frame=1)
    assert not res["bad"], res["bad"][:1]
    assert res["wide"] <= 0.01 * res["rays"] and res["kinds"] == {0, 1, 2, 3, 4} and 0.05 <= res["ratio"] <= 1.0
    world = scan_scene(sc, None, RMAX, PED, POINT, directions=dirs)
    assert np.array_equal(rec[6], world[6]) and sum((rec[i] != world[i]).any() for i in range(65)) >= 60
    assert len(_check(sc, dirs, RMAX, PED, POINT, frame=1, rec=world)[1]["bad"]) > 500    # the world-frame record is far outside


# ---- 4. exact translation -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", [0, 1])
def test_translation_by_a_representable_shift_is_exact(frame):
    """Coordinates on a grid of 2^-10 m, shifted by (+4096, -8192): every ax, ay and goal entry is the same float, so the record
    is the same bits."""
    near = T.quantised(_crowd(65, False))
    far = T.shifted(near)
    for sc in (near, far):
        pk = pack_scenes([sc])
        for key in ("x", "y", "wx", "wy"):
            assert np.array_equal(pk[key].astype(np.float64) * 1024, np.round(pk[key].astype(np.float64) * 1024)), key
    a = scan_scene(near, default_angles(33), RMAX, PED, POINT, frame=frame)
    b = scan_scene(far, default_angles(33), RMAX, PED, POINT, frame=frame)
    assert (a[:, 33:] > 0).any() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 5. copies of the twin with one line changed --------------------------------------------------------------------------------

# The five copies the issue names -- s = t + w, no clamp at 0, r for r2, the frame-1 rotation transposed, static and vehicle kinds
# swapped -- are each refused by an analytic case of test_batch_scan_host.py already (in turn: test_a_disc_dead_ahead_and_the_same_
# disc_behind, test_inside_a_disc_the_range_is_zero, test_a_disc_dead_ahead_and_the_same_disc_behind, test_heading_frame,
# test_order_rule_and_every_kind), so they are not repeated here.  Those cases all look straight at a disc's centre (c = 0): a copy
# that is only wrong off the centre line passes every one of them.
MUTATIONS = {                                                            # name: (the twin's line, the changed line)
    "the chord forgotten": ("w = np.sqrt(q)", "w = np.sqrt(np.where(q > 0, r2[None, :], q))"),
    "half the chord": ("w = np.sqrt(q)", "w = np.sqrt(np.where(q > 0, _fma32(-c, c * np.float32(0.5), r2[None, :]), q))"),
}
OLD_HOST_TESTS = ("test_a_disc_dead_ahead_and_the_same_disc_behind", "test_inside_a_disc_the_range_is_zero",
                  "test_order_rule_and_every_kind", "test_a_range_equal_to_max_range_is_a_miss", "test_radius_zero_switches_a_kind_off",
                  "test_ghost_rows_and_nan_rows_are_zero_and_unseen", "test_mask_and_state_and_3d", "test_heading_frame",
                  "test_rotating_the_rays_rotates_the_record", "test_twin_refuses_bad_settings")


def _mutant(name):
    old, new = MUTATIONS[name]
    src = inspect.getsource(S._disc_ranges)
    assert src.count(old) == 1, name
    ns = dict(vars(S))
    exec(compile(src.replace(old, new), f"<scan._disc_ranges: {name}>", "exec"), ns)
    return ns["_disc_ranges"]


def _old_tests_pass():
    try:
        for t in OLD_HOST_TESTS:
            getattr(H, t)()
        for frame in (0, 1):
            H.test_pruning_changes_nothing(frame)
    except AssertionError:
        return False
    return True


def _new_tests_pass():
    with np.errstate(all="ignore"):
        if T.check(scan_scene(_crowd(17, False), default_angles(33), RMAX, PED, POINT), pack_scenes([_crowd(17, False)]), 0,
                   ray_directions(default_angles(33)), RMAX, PED, POINT)["bad"]:
            return False
        sc = _crowd(17, True)
        rec = scan_scene(sc, default_angles(33), RMAX, PED, POINT, frame=1)
        return not T.check(rec, pack_scenes([sc]), 0, ray_directions(default_angles(33)), RMAX, PED, POINT, frame=1)["bad"]


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_a_twin_with_one_line_changed_is_refused(name, monkeypatch):
    """Every changed copy must leave the envelope on the smallest crowd (frame 0 at the origin, frame 1 shifted) while the analytic
    cases and the pruning test of test_batch_scan_host.py still pass."""
    assert _old_tests_pass() and _new_tests_pass()                       # the twin itself passes both
    monkeypatch.setattr(S, "_disc_ranges", _mutant(name))
    assert not _new_tests_pass(), f"{name}: inside the envelope"
    assert _old_tests_pass(), f"{name}: refused by test_batch_scan_host.py already"
