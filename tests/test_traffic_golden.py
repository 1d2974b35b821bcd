"""Gap acceptance and vehicle rings against outputs of the reference's own check_traffic.check_traffic and
obstacles.generate_ellipse_border (tests/golden/traffic/*.npz, written by tests/golden/make_golden_traffic.py; inputs rebuilt
from tests/_traffic_cases.py and guarded by a digest).  SURVEY.md section 8f rows 2 and 3: the reference's control flow and
arithmetic are pinned; what is still taken on trust is the stand-ins' definition of two library primitives (segment
intersection / distance, a yaw rotation), which the first tests here hold to hand-derived cases."""
import importlib.util
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import _golden_io as gio
import _traffic_cases as TC
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd.check_traffic import check_traffic
from oracle import sfm_oracle as O

TRAFFIC_DIR = os.path.join(gio.GOLDEN_DIR, "traffic")
STANDINS = os.path.join(gio.GOLDEN_DIR, "_standins")


def _load(name):
    z = np.load(os.path.join(TRAFFIC_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _standin(name, path):
    spec = importlib.util.spec_from_file_location("_standin_" + name, os.path.join(STANDINS, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_shapely_stand_in_on_hand_derived_cases():
    g = _standin("geometry", os.path.join("shapely", "geometry.py"))
    L, P = g.LineString, g.Point
    a = L([(0, 0), (8, 0)])
    x = a.intersection(L([(4, -3), (4, 5)]))                                   # a crossing
    assert not x.is_empty and (x.distance(P((4, 0))), x.distance(P((0, 0))), x.distance(P((4, -3)))) == (0.0, 4.0, 3.0)
    assert a.intersection(L([(4, 0.5), (4, 5)])).is_empty                      # stops short
    t = a.intersection(L([(8, 0), (8, 5)]))                                    # T-touch at an end point of both
    assert not t.is_empty and t.distance(P((8, 0))) == 0.0 and t.distance(P((5, 4))) == 5.0
    assert a.intersection(L([(0, 1), (8, 1)])).is_empty                        # parallel
    assert a.intersection(L([(9, 0), (12, 0)])).is_empty                       # collinear, disjoint
    p = a.intersection(L([(8, 0), (12, 0)]))                                   # collinear, one point
    assert (p.distance(P((8, 0))), p.distance(P((0, 0)))) == (0.0, 8.0)
    s = a.intersection(L([(12, 0), (6, 0)]))                                   # collinear overlap [6, 8]
    assert (s.distance(P((0, 0))), s.distance(P((7, 0))), s.distance(P((7, 2))), s.distance(P((11, 4)))) == (6.0, 0.0, 2.0, 5.0)
    # no tolerance: one float64 ulp off the end is a miss, a crossing on non-representable thirds is found
    assert a.intersection(L([(np.nextafter(8.0, 9.0), -1), (np.nextafter(8.0, 9.0), 1)])).is_empty
    third = L([(0, 0), (3, 1)]).intersection(L([(1, 1), (1, -1)]))
    assert abs(third.distance(P((1, 0))) - 1.0 / 3.0) < 1e-16
    assert L([(0, 0), (1, 1)]).intersection(L([(2, 0), (0, 2)])).distance(P((0, 0))) == np.sqrt(2.0)
    z = L([(4, 0), (4, 0)])                                                    # a zero-length line is its point
    assert not z.intersection(L([(4, -1), (4, 1)])).is_empty and z.intersection(L([(5, -1), (5, 1)])).is_empty
    assert z.intersection(L([(4, 1), (4, 2)])).is_empty
    with pytest.raises(NotImplementedError):
        L([(0, 0), (1, 0), (2, 0)])


def test_carla_stand_in_on_hand_derived_cases():
    c = _standin("carla", "carla.py")
    q = c.Transform(c.Location(10.0, -20.0, 1.0), c.Rotation(yaw=90.0)).transform(c.Location(2.0, 0.5, 0.0))
    assert np.allclose((q.x, q.y, q.z), (9.5, -18.0, 1.0), atol=1e-15)         # rotate (x -> y), then translate
    q = c.Transform(c.Location(1.0, 2.0, 3.0), c.Rotation(yaw=180.0)).transform(c.Location(1.0, 0.0, 0.0))
    assert np.allclose((q.x, q.y, q.z), (0.0, 2.0, 3.0), atol=1e-15)
    q = c.Transform(c.Location(), c.Rotation(yaw=30.0)).transform(c.Location(2.0, 0.0, 0.0))
    assert np.allclose((q.x, q.y), (np.sqrt(3.0), 1.0), atol=1e-15)


def _cases(name):
    cs = TC.random_cases() if name == "gap_random" else TC.exact_cases()
    fx = _load(name)
    assert TC.digest(cs) == str(fx["digest"]), f"{name}: tests/_traffic_cases.py no longer builds the inputs the fixture was written for"
    assert len(fx["decision"]) == len(cs["loc"]) == len(fx["slack"])
    return cs, fx


def _decide_both(cs):
    """(oracle decision, product host function decision) per case, the host function called as the reference's call site does."""
    C = len(cs["loc"])
    ora, host = np.zeros(C, bool), np.zeros(C, bool)
    for g in range(len(cs["group_off"]) - 1):
        vl, vv, ve, sl = TC.group(cs, g)
        vehicles = [(v, None) for v in vl]
        for i in range(sl.start, sl.stop):
            ora[i] = O.gap_accepted(cs["loc"][i], cs["goal"][i], cs["speed"][i], cs["margin"][i], vl, vv, ve)
            ped = {"loc": np.append(cs["loc"][i], 0.0), "next_waypoint": np.append(cs["goal"][i], 0.0),
                   "mode": SimpleNamespace(crossing_speed=float(cs["speed"][i]), crossing_safety_margin=float(cs["margin"][i]))}
            host[i] = check_traffic(ped, vehicles, vv, list(ve))
    return ora, host


def _mismatches(cs, fx, got, mask):
    bad = np.nonzero(mask & (got != fx["decision"].astype(bool)))[0]
    return [f"{TC.describe(cs, i)}: reference {bool(fx['decision'][i])}, slack {fx['slack'][i]:.3g}" for i in bad[:5]], len(bad)


def test_random_decisions_match_the_reference():
    cs, fx = _cases("gap_random")
    decided = fx["slack"] >= TC.SLACK_BAND
    undecided = 1.0 - decided.mean()
    refused = (fx["decision"] == 0).mean()
    print(f"random class: {len(decided)} cases, {100 * undecided:.2f} % undecided, {100 * refused:.1f} % refused")
    assert undecided <= TC.UNDECIDED_CAP
    assert 0.10 <= refused <= 0.40                                             # "always accept" cannot pass
    assert (fx["decision"][cs["margin"] < 0] == 1).all()
    for who, got in zip(("oracle", "host"), _decide_both(cs)):
        msgs, n = _mismatches(cs, fx, got, decided)
        assert n == 0, f"{who}: {n} decided cases differ from the reference\n" + "\n".join(msgs)
        print(f"{who}: {int((got != fx['decision'].astype(bool))[~decided].sum())} of {int((~decided).sum())} undecided cases differ")
    # the recorded slack is the oracle's (fp32 in the file)
    for i in np.random.default_rng(1).choice(len(decided), 200, replace=False):
        vl, vv, ve, _ = TC.group(cs, int(TC.group_of_case(cs)[i]))
        s = np.float32(O.gap_slack(cs["loc"][i], cs["goal"][i], cs["speed"][i], cs["margin"][i], vl, vv, ve))
        assert s == fx["slack"][i], TC.describe(cs, i)


def test_exact_and_degenerate_decisions_match_the_reference():
    cs, fx = _cases("gap_exact")
    kinds = np.array(TC.KINDS)[cs["kind"]]
    assert set(kinds) == set(TC.KINDS[1:])                                     # every named case is there
    for k in ("tie_front", "tie_back", "touch_t1_u1"):                         # strict inequalities: a tie accepts
        assert (fx["decision"][kinds == k] == 1).all(), k
    for k in ("next_to_tie_front", "next_to_tie_back", "touch_t1", "stationary_then_refusing"):
        assert (fx["decision"][kinds == k] == 0).all(), k
    for k in ("first_extent_decides", "diagonal_extent_product", "standing_on_path", "touch_t0", "touch_u0", "collinear_overlap"):
        d = fx["decision"][kinds == k]
        assert 0 < d.sum() < len(d), k                                         # both outcomes
    degenerate = np.isin(kinds, TC.DEGENERATE_KINDS)
    if str(fx["backend"][0]).startswith("stand-in"):
        assert np.array_equal(fx["project_defined"].astype(bool), degenerate)
    for i in np.nonzero(~degenerate)[0]:                                       # the claims the builder makes, case by case
        if kinds[i] in TC.EXACT_KINDS:
            assert TC.assert_exact(cs, i) == bool(fx["decision"][i]), TC.describe(cs, i)
        else:
            assert fx["slack"][i] >= TC.ROBUST_SLACK, TC.describe(cs, i)
    ora, host = _decide_both(cs)
    for who, got in (("oracle", ora), ("host", host)):                         # no band: every case, the degenerate ones included
        msgs, n = _mismatches(cs, fx, got, np.ones(len(got), bool))
        assert n == 0, f"{who}: {n} exact cases differ from the reference\n" + "\n".join(msgs)
    assert np.array_equal(ora[degenerate], host[degenerate])                   # one answer, whoever defined it


def test_a_flipped_decision_is_noticed():
    cs, fx = _cases("gap_exact")
    fx = dict(fx, decision=fx["decision"].copy())
    fx["decision"][17] ^= 1
    assert _mismatches(cs, fx, _decide_both(cs)[0], np.ones(len(cs["loc"]), bool))[1] == 1


@pytest.mark.parametrize("name", ["random", "edge"])
def test_rings_match_the_reference(name):
    center, yaw, extent = TC.ring_cases()[name]
    fx = _load("rings_" + name)
    assert TC.digest(TC.ring_inputs((center, yaw, extent))) == str(fx["digest"]), "ring inputs drifted"
    off = np.concatenate([[0], np.cumsum(fx["count"])])
    assert off[-1] == len(fx["points"])
    if name == "edge":
        lo, mid, hi = (fx["count"][k:-6:3] for k in range(3))                   # circumference from below, nearest, from above
        assert (hi - lo == 1).all() and (mid == lo).any() and (mid == hi).any()  # the count is the edge: n - 1, then n
        assert (fx["count"][-6:] == 6).sum() >= 5                               # the floor
    worst = [0.0, 0.0, 0.0]
    for k in range(len(center)):
        want = fx["points"][off[k]:off[k + 1]]
        ex, ey = extent[k]
        got = (O.ellipse_ring(center[k], yaw[k], ex, ey), scenarios.ellipse_ring(center[k], yaw[k], ex, ey),
               scenarios.place_ring_f32(center[k], yaw[k], scenarios.ring_local_offsets(ex, ey)))
        for q, (g, tol) in enumerate(zip(got, (1e-9, 1e-4, 1e-4))):
            assert g.shape == want.shape, f"vehicle {k}: {g.shape[0]} points, the reference made {fx['count'][k]} (extent {ex!r}, {ey!r})"
            worst[q] = max(worst[q], float(np.max(np.abs(g - want))))
            assert worst[q] <= tol, f"vehicle {k} (centre {center[k].tolist()}, yaw {yaw[k]!r}): {worst[q]:.3g} > {tol}"
    print(f"rings {name}: worst |oracle - ref| {worst[0]:.2e}, |scenarios.ellipse_ring - ref| {worst[1]:.2e}, |fp32 placement - ref| {worst[2]:.2e}")


def test_committed_digests_are_what_the_generator_builds_today(tmp_path):
    gen = os.path.join(gio.GOLDEN_DIR, "make_golden_traffic.py")
    subprocess.check_call([sys.executable, gen, "--inputs-only", "--out", str(tmp_path)], stdout=subprocess.DEVNULL)
    names = sorted(f[:-4] for f in os.listdir(TRAFFIC_DIR) if f.endswith(".npz"))
    assert names == ["gap_exact", "gap_random", "rings_edge", "rings_random"]
    for name in names:
        new = np.load(tmp_path / (name + ".npz"), allow_pickle=False)
        assert str(new["digest"]) == str(_load(name)["digest"]), name
        assert os.path.getsize(os.path.join(TRAFFIC_DIR, name + ".npz")) < 144 * 1024, name
