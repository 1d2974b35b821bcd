"""Host tests of the row episodes' and row respawns' NumPy twins (episode.row_episode_scene, reset.respawn_rows_scene): what the
device is compared against bit for bit in tests/test_batch_row_episodes_gpu.py is itself pinned here -- to episode_scene where there
is one agent, to the rules at their edges, to float64 distances within the bound derived in tests/_row_episode_cases.py, and to the
restart noise's rule with the three changes of a respawn.  No GPU, no library."""
import numpy as np
import pytest

import _row_episode_cases as RC
from carla_social_force_model_amd import episode as E, reset as R

F = np.float32


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _scene(loc, wp, borders=None, static=None, vehicles=None):
    loc, wp = np.asarray(loc, dtype=np.float64), np.asarray(wp, dtype=np.float64)
    return {"loc": loc, "vel": np.zeros_like(loc), "waypoint": wp, "borders": borders or [], "static_obstacles": static or [],
            "dynamic_obstacles": vehicles or []}


# ---- H1 ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", sorted(RC.ONE))
def test_one_agent_reduces_to_episode_scene(k):
    sc, a = RC.scenes()[k], RC.ONE[k]
    flags = RC.agents()[k]
    assert flags.sum() == 1 and flags[a]
    radii = (RC.GOAL_R[k], RC.PED_R[k], RC.VEH_R[k])
    loc, vel = sc["loc"].copy(), sc["vel"]
    age, prev, ages, prevs = 0, np.nan, None, None
    for step in range(3):                                              # the first evaluation starts from a NaN prev
        state = (loc, vel)
        want, (age, prev) = E.episode_scene(sc, a, radii, RC.MAX_STEPS[k], age, prev, state=state)
        rec, done, ages, prevs = E.row_episode_scene(sc, flags, radii, RC.MAX_STEPS[k], ages, prevs, state=state)
        assert np.array_equal(_bits(rec[a]), _bits(want)), step
        assert done[a] == bool(want[E.EP_DONE]) and ages[a] == age
        assert np.array_equal(_bits(prevs[a]), _bits(prev))
        others = ~flags
        assert not rec[others].any() and not done[others].any() and not ages[others].any() and np.isnan(prevs[others]).all()
        loc = np.float32(loc + 0.2 * vel).astype(np.float64)          # the crowd moves between the evaluations
    assert rec[a, E.EP_PREV_GOAL_D2] != rec[a, E.EP_GOAL_D2]


# ---- H2 ---------------------------------------------------------------------------------------------------------------------------------

def _below(v):
    return np.nextafter(F(v), F(0))


def test_strictness_at_exactly_the_radius_and_one_ulp_inside():
    # agent 0 at the origin; a neighbour, a ring point and the goal each at distance 2 exactly (d2 = 4 = r2 for r = 2)
    ring = np.array([[0.0, 2.0], [0.0, 5.0], [1.0, 5.0]])
    sc = _scene([[0, 0, 0], [2, 0, 0]], [[0, -2, 0], [50, 50, 0]], vehicles=[(np.array([0.0, 4.0]), ring)])
    rec, done, _, _ = E.row_episode_scene(sc, [1, 0], (2.0, 2.0, 2.0), 0)
    assert rec[0, E.EP_GOAL_D2] == 4 and rec[0, E.EP_PED_D2] == 4 and rec[0, E.EP_VEH_D2] == 4
    assert rec[0, E.EP_REASON] == 0 and not done[0]
    for slot, bit, move in ((E.EP_PED_D2, E.REASON_PED_HIT, "ped"), (E.EP_VEH_D2, E.REASON_VEH_HIT, "veh"), (E.EP_GOAL_D2, E.REASON_ARRIVED, "goal")):
        loc, wp, rg = np.array([[0, 0, 0], [2, 0, 0]], float), np.array([[0, -2, 0], [50, 50, 0]], float), ring.copy()
        if move == "ped":
            loc[1, 0] = _below(2.0)
        elif move == "veh":
            rg[0, 1] = _below(2.0)
        else:
            wp[0, 1] = -_below(2.0)
        rec, done, _, _ = E.row_episode_scene(_scene(loc, wp, vehicles=[(np.array([0.0, 4.0]), rg)]), [1, 0], (2.0, 2.0, 2.0), 0)
        assert rec[0, slot] < 4 and rec[0, E.EP_REASON] == bit and done[0], move


def test_radius_zero_never_fires_and_the_time_limit_does():
    sc = _scene([[1, 1, 0], [1, 1, 0]], [[1, 1, 0], [1, 1, 0]], vehicles=[(np.array([1.0, 1.0]), np.array([[1.0, 1.0], [1.0, 2.0], [2.0, 2.0]]))])
    rec, done, ages, _ = E.row_episode_scene(sc, True, (0.0, 0.0, 0.0), 2)
    assert (rec[:, [E.EP_GOAL_D2, E.EP_PED_D2, E.EP_VEH_D2]] == 0).all() and not done.any() and (rec[:, E.EP_REASON] == 0).all()
    rec, done, ages, _ = E.row_episode_scene(sc, True, (0.0, 0.0, 0.0), 2, ages=ages)
    assert done.all() and (rec[:, E.EP_REASON] == E.REASON_TIME_LIMIT).all() and (ages == 2).all()


@pytest.mark.parametrize("bad", [RC.FAR, np.nan])
def test_an_agent_that_is_not_live(bad):
    sc = _scene([[bad, 0, 0], [1, 0, 0], [2, 0, 0]], [[5, 5, 0]] * 3)
    prevs = np.array([7.5, np.nan, np.nan], F)
    rec, done, ages, prevs = E.row_episode_scene(sc, [1, 1, 0], (1.0, 1.0, 1.0), 0, prevs=prevs)
    assert rec[0, E.EP_REASON] == E.REASON_NOT_LIVE and done[0] and np.isposinf(rec[0, 3:8]).all() and prevs[0] == F(7.5)
    assert rec[1, E.EP_PED_D2] == 1 and not done[1]                    # the row that is not live is in nobody's way: row 2 is nearest
    assert not rec[2].any()


def test_two_agents_at_the_same_place_hit_each_other():
    sc = _scene([[3, 4, 0], [3, 4, 0], [30, 40, 0]], [[9, 9, 0]] * 3)
    rec, done, _, _ = E.row_episode_scene(sc, [1, 1, 1], (0.0, 0.5, 0.0), 0)
    assert (rec[:2, E.EP_PED_D2] == 0).all() and (rec[:2, E.EP_REASON] == E.REASON_PED_HIT).all() and done[:2].all() and not done[2]


# ---- H3 ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 6, 10, 11])
def test_distance_slots_are_minima_of_the_true_distances_within_the_bound(k):
    sc = RC.scenes()[k]
    rec, _, _, _ = RC.twin(k, (sc["loc"], sc["vel"]), sc["waypoint"], None)
    xy = np.asarray(sc["loc"], dtype=np.float32).astype(np.float64)[:, :2]
    live = (np.abs(xy) < 1e12).all(axis=1)
    from carla_social_force_model_amd.observe import _polylines
    vp = _polylines(sc["dynamic_obstacles"] or [], True)[0].astype(np.float64)
    wp = np.concatenate([_polylines(sc["borders"] or [], False)[0], _polylines(sc["static_obstacles"] or [], True)[0]]).astype(np.float64)
    checked = 0
    for i in np.flatnonzero(RC.agents()[k] & live):
        others = live.copy()
        others[i] = False
        for slot, cand in ((E.EP_PED_D2, xy[others]), (E.EP_VEH_D2, vp), (E.EP_WALL_D2, wp)):
            if len(cand) == 0:
                assert np.isposinf(rec[i, slot])
                continue
            true = ((cand - xy[i]) ** 2).sum(axis=1).min()
            assert abs(float(rec[i, slot]) - true) <= RC.REL_D2 * true, (i, slot)
            checked += 1
    assert checked > 0


def test_the_bound_is_the_one_derived():
    assert RC.REL_D2 == (1 + 2.0 ** -24) ** 4 - 1 and 0.999999 < RC.GAP_SLACK < 1
    assert [RC.split(int(a.sum())) for a in RC.agents() if a.any()] == [RC.SPLIT[k] for k, a in enumerate(RC.agents()) if a.any()]
    assert sorted(set(RC.SPLIT.values())) == [1, 2, 4, 8, 16, 32, 64]               # every value of the split


# ---- H4 ---------------------------------------------------------------------------------------------------------------------------------

def _moved(k, seed):
    """A 'now' for scene k: the crowd shifted and shuffled a little, waypoints changed."""
    sc = RC.scenes()[k]
    rng = np.random.default_rng(seed)
    n = sc["loc"].shape[0]
    loc = np.float32(sc["loc"] + np.c_[rng.uniform(-0.4, 0.4, (n, 2)), np.zeros(n)]).astype(np.float64)
    vel = np.float32(sc["vel"] * 0.5).astype(np.float64)
    wp = np.float32(sc["waypoint"][:, :2] + 1.0).astype(np.float64)
    return (loc, vel), wp


@pytest.mark.parametrize("k", [3, 6, 10])
def test_respawn_without_noise_is_snapshot_rows_for_the_chosen_and_current_rows_for_the_rest(k):
    sc = RC.scenes()[k]
    snap = ((sc["loc"], sc["vel"]), sc["waypoint"][:, :2])
    now = _moved(k, 5)
    ch = RC.chosen(0)[k]
    loc, vel, wp, resets, fb = RC.respawn_twin(k, ch, snap, now, noise=False)
    assert fb is None and not resets.any()
    assert np.array_equal(loc[ch], F(sc["loc"][ch])) and np.array_equal(vel[ch], F(sc["vel"][ch])) and np.array_equal(wp[ch], F(sc["waypoint"][ch, :2]))
    assert np.array_equal(loc[~ch], F(now[0][0][~ch])) and np.array_equal(vel[~ch], F(now[0][1][~ch])) and np.array_equal(wp[~ch], F(now[1][~ch]))
    assert ch.any() and (~ch).any()


def test_respawn_words_differ_from_restart_words():
    i, t = np.meshgrid(np.arange(64), np.arange(8))
    for e in (0, 1, 5):
        for c in range(4):
            a, b = R.respawn_word(77, i, e, t, c), R.reset_word(77, i, e, t, c)
            assert a.dtype == np.uint32 and (a != b).all()
    assert (R.respawn_word(77, 3, np.arange(100), 0, 0)[1:] != R.respawn_word(77, 3, 0, 0, 0)).all()      # never repeats over e


def _pair_scene(gap_to_now):
    """Rows 0, 1, 2 on a line 10 m apart in the snapshot; NOW row 2 stands ``gap_to_now`` from row 1's snapshot position."""
    s_loc = np.array([[0.0, 0, 0], [10.0, 0, 0], [20.0, 0, 0]])
    n_loc = s_loc.copy()
    n_loc[2, 0] = 10.0 + gap_to_now
    sc = _scene(s_loc, [[0, 5, 0]] * 3)
    return sc, ((s_loc, np.zeros((3, 3))), sc["waypoint"][:, :2]), ((n_loc, np.zeros((3, 3))), sc["waypoint"][:, :2])


def test_rejection_is_against_a_row_that_is_not_chosen_where_it_stands_now():
    sc, snap, now = _pair_scene(0.05)
    box = np.array([[0, 0], [0.02, 0.02], [0, 0]])
    kw = dict(seed=9, pos_box=box, min_gap=0.5, tries=4, detail=True)
    out = R.respawn_rows_scene(sc, [0, 1, 0], snap[0], snap[1], now[0], now[1], **kw)
    assert out[4] == 1 and out[5]["rejected"]["blocker"] == 4 and out[5]["round"][1] == R.FALLBACK     # row 2 stands on the box NOW
    assert np.array_equal(out[0][1], F([10, 0, 0]))                                                      # the fallback: the snapshot position
    out = R.respawn_rows_scene(sc, [0, 1, 0], snap[0], snap[1], snap[0], snap[1], **kw)                 # ... at its snapshot position it is 10 m away
    assert out[4] == 0 and out[5]["rejected"]["blocker"] == 0 and out[5]["round"][1] == 0
    assert list(out[3]) == [0, 1, 0]


def test_a_forced_fallback_is_counted_and_the_lower_index_rule_holds_between_chosen_rows():
    sc, snap, now = _pair_scene(0.0)
    box = np.array([[0, 0], [0.01, 0.01], [0, 0]])
    out = R.respawn_rows_scene(sc, [0, 1, 0], snap[0], snap[1], now[0], now[1], seed=3, pos_box=box, min_gap=0.3, tries=1, detail=True)
    assert out[4] == 1 and out[5]["round"][1] == R.FALLBACK
    # two chosen rows whose boxes overlap entirely: the higher index is rejected against the lower's proposal, never the reverse
    s_loc = np.array([[0.0, 0, 0], [0.0, 0, 0]])
    sc2 = _scene(s_loc, [[1, 1, 0]] * 2)
    st = (s_loc, np.zeros((2, 3)))
    out = R.respawn_rows_scene(sc2, [1, 1], st, sc2["waypoint"][:, :2], st, sc2["waypoint"][:, :2], seed=4, pos_box=[0.05, 0.05], min_gap=1.0, tries=3,
                               detail=True)
    assert out[5]["round"][0] == 0 and out[5]["round"][1] == R.FALLBACK and out[5]["rejected"] == {"blocker": 2, "lower": 1, "point": 0}
    assert out[4] == 1 and list(out[3]) == [1, 1]


@pytest.mark.parametrize("k", RC.PROPERTY_SCENES)
def test_property_scenes_place_every_row_and_keep_the_gaps_in_float64(k):
    sc = RC.scenes()[k]
    snap = ((sc["loc"], sc["vel"]), sc["waypoint"][:, :2])
    now = _moved(k, 11) + (sc["dynamic_obstacles"],)
    ch = RC.chosen(0)[k]
    loc, _, _, resets, fb, info = RC.respawn_twin(k, ch, snap, now, detail=True, **RC.PROPERTY_GAPS)
    assert fb == 0                                                     # asserted, not skipped: the cases are chosen so that it holds
    placed = np.flatnonzero(info["round"] >= 0)
    assert len(placed) > 0 and np.array_equal(resets, ch.astype(np.uint32))
    live = (np.abs(loc[:, :2]) < 1e12).all(axis=1)
    dp, dq = RC.min_true_distances(loc[:, :2], placed, live, RC.scene_points(k))
    assert (dp >= RC.PROPERTY_GAPS["min_gap"] * RC.GAP_SLACK).all() and (dq >= RC.PROPERTY_GAPS["point_gap"] * RC.GAP_SLACK).all()


def test_the_dense_setting_rejects_under_every_condition():
    """The crowd of the GPU comparison is not a trivial one: over the three respawns every kind of rejection and a fallback occur."""
    total = {"blocker": 0, "lower": 0, "point": 0}
    late = fallbacks = 0
    for k in (3, 7, 9, 10):
        sc = RC.scenes()[k]
        snap = ((sc["loc"], sc["vel"]), sc["waypoint"][:, :2])
        now = _moved(k, 21) + (sc["dynamic_obstacles"],)
        for step in (0, 1):
            out = RC.respawn_twin(k, RC.chosen(step)[k], snap, now, detail=True)
            for key in total:
                total[key] += out[5]["rejected"][key]
            late += int((out[5]["round"] > 0).sum())
            fallbacks += out[4] or 0
            if k == RC.STUCK_SCENE and step == 1:
                assert out[5]["round"][1] == R.FALLBACK               # the designed row
    assert all(v > 0 for v in total.values()) and late > 0 and fallbacks > 0


def test_the_example_imports_without_a_gpu():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("batch_multiagent_loop", os.path.join(root, "examples", "batch_multiagent_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.run) and callable(mod.make_policy) and callable(mod.rewards)
