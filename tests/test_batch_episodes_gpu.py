"""GPU tests of the batch's episode ends and the restart by device mask (sfm_batch_set_episodes, sfm_batch_end_step,
sfm_batch_download_episodes, sfm_batch_restart_device; SfmBatch.set_episodes / end_step / episodes / episode_tensor / done_tensor /
restart_device): the record bitwise against the host twin ``episode.episode_scene``, the strict ``<`` of every rule on its edge,
independence of the rest of the batch, planar against 3-D, that an evaluation changes nothing a tick computes, the device-mask
restart against the host-mask restart in everything that can be read back, the auto restart against a host-driven loop, the device
views, and every refusal.  Every comparison is bitwise.  Run on the MI355X box with  python -m pytest tests -m gpu."""
import importlib.util
import os
from functools import lru_cache

import numpy as np
import pytest

import test_batch_gpu as G
import test_batch_modes_gpu as M
import test_batch_restart_gpu as R
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd._lib import SfmLibraryError
from carla_social_force_model_amd.batch import (EP_AGE, EP_DONE, EP_GOAL_D2, EP_PED_D2, EP_PREV_GOAL_D2, EP_REASON, EP_VEH_D2,
                                                EP_WALL_D2, PTR_DONE, PTR_EPISODES, REASON_ARRIVED, REASON_NOT_LIVE,
                                                REASON_PED_HIT, REASON_TIME_LIMIT, REASON_VEH_HIT, SfmBatch)
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.episode import episode_scene
from test_batch_episodes_host import JUST_ABOVE_5, bare, ring

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3
INF = np.float32(np.inf)
# one lane, a wave boundary, a workgroup boundary, several strides, an empty scene; the last two carry 3 device-side vehicles each
SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1024, 40, 90)
STAGES = (0, 1, 5)                       # integrating ticks before the three end_step calls
GOAL_R, PED_R, VEH_R = (3.0, 6.0, 0.0), (0.5, 0.0, 1.1), (1.5, 0.0, 4.0)      # per scene in turn; 0: the test is off
MAX_STEPS = (0, 2, 5)


def _agents(sizes):
    return [-1 if n == 0 else (0, n - 1, n // 2)[q % 3] for q, n in enumerate(sizes)]


def _settings(B):
    pick = lambda vals: [vals[q % len(vals)] for q in range(B)]
    return pick(GOAL_R), pick(PED_R), pick(VEH_R), pick(MAX_STEPS)


@lru_cache(maxsize=None)
def _scenes(z3=False):
    """The mixed batch.  The 3-D form has the planar form's x, y, vx, vy, with a z and a vz of its own per row."""
    scenes = [G._scene(n, 6000 + q, dynamic=3 if q >= len(SIZES) - 2 else 0) for q, n in enumerate(SIZES)]
    if z3:
        rng = np.random.default_rng(6)
        for sc in scenes:
            n = len(sc["loc"])
            sc["loc"] = np.column_stack([sc["loc"][:, :2], rng.uniform(0.0, 1.5, n)])
            sc["vel"] = np.column_stack([sc["vel"][:, :2], rng.uniform(-0.2, 0.2, n)])
    return scenes


def _batch(scenes, device_vehicles=True, episodes=True, agents=None, cfg=None):
    b = SfmBatch(cfg or default_sfm_config(scenarios.ALL_FORCES), 0.05, B=len(scenes))
    try:
        b.upload(scenes, device_vehicles=device_vehicles)
        if episodes:
            b.set_episodes(_agents([len(sc["loc"]) for sc in scenes]) if agents is None else agents, *_settings(len(scenes)))
    except Exception:
        b.close()
        raise
    return b


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: {got} != {want}"


def _twin_rows(b, scenes, agents, settings, ages, prevs):
    """episode_scene of every scene on what the device holds now; ages / prevs are advanced in place."""
    rg, rp, rv, ms = settings
    rows = []
    for q, (sc, st, veh, (wp, _)) in enumerate(zip(scenes, b.state(), b.dynamic_obstacles(), b.waypoints())):
        rec, (ages[q], prevs[q]) = episode_scene(sc, agents[q], (rg[q], rp[q], rv[q]), ms[q], ages[q], prevs[q], state=st,
                                                 vehicles=veh, waypoints=wp)
        rows.append(rec)
    return np.stack(rows)


@lru_cache(maxsize=None)
def _staged(z3, only=None):
    """The mixed batch (or its scene ``only`` alone, with that scene's settings): (device records, device done, twin records)
    after each of STAGES."""
    scenes = _scenes(z3)
    B = len(scenes)
    agents, settings = _agents(SIZES), _settings(B)
    if only is not None:
        scenes, agents, settings = [scenes[only]], [agents[only]], tuple([s[only]] for s in settings)
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), 0.05, B=len(scenes))
    try:
        b.upload(scenes, device_vehicles=True)
        assert b.planar == (not z3)
        b.set_episodes(agents, *settings)
        ages, prevs = [0] * len(scenes), [np.nan] * len(scenes)
        out, ran = [], 0
        for t in STAGES:
            b.run(t - ran)
            ran = t
            b.end_step()
            rec, done = b.episodes()
            out.append((rec, done, _twin_rows(b, scenes, agents, settings, ages, prevs)))
        return out
    finally:
        b.close()


# ---- 1. bitwise against the twin ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
def test_the_record_is_bitwise_the_twin(z3):
    """After 0, 1 and 5 integrating ticks, three end_step calls in a row: record and done of every scene, the age (1, 2, 3) and the
    carried prev_goal_d2 included."""
    stages = _staged(z3)
    agents = _agents(SIZES)
    for k, (rec, done, want) in enumerate(stages):
        assert rec.shape == (len(SIZES), 8) and done.shape == (len(SIZES),) and done.dtype == bool
        for q in range(len(SIZES)):
            _same_bits(rec[q], want[q], f"stage {k}, scene {q} (N = {SIZES[q]}, agent {agents[q]})")
        assert np.array_equal(done, want[:, EP_DONE] != 0)
        assert np.array_equal(rec[:, EP_AGE], np.full(len(SIZES), k + 1, np.float32))
        live = np.array(agents) >= 0
        assert np.isfinite(rec[live, EP_GOAL_D2]).all() and (rec[~live, EP_GOAL_D2:] == INF).all()
        if k:                                                           # prev is the goal distance of the evaluation before
            assert np.array_equal(rec[live, EP_PREV_GOAL_D2], stages[k - 1][0][live, EP_GOAL_D2])
        else:
            assert np.array_equal(rec[live, EP_PREV_GOAL_D2], rec[live, EP_GOAL_D2])
    # the batch holds every class of scene, by the twin alone
    first, last = stages[0][2], stages[-1][2]
    assert (last[:, EP_DONE] == 1).any() and (last[:, EP_DONE] == 0).any()
    reasons = np.bitwise_or.reduce(np.concatenate([s[2][:, EP_REASON] for s in stages]).astype(np.int64))
    assert reasons & REASON_ARRIVED and reasons & REASON_TIME_LIMIT and reasons & REASON_PED_HIT and reasons & REASON_VEH_HIT
    assert np.isfinite(first[-2:, EP_VEH_D2]).all() and (first[:-2, EP_VEH_D2] == INF).all()
    assert first[1, EP_PED_D2] == INF and np.isfinite(first[2:, EP_PED_D2]).all()              # N_b = 1 has nobody to touch
    assert np.isfinite(first[1:, EP_WALL_D2]).all()
    assert not np.array_equal(first[:, EP_GOAL_D2], last[:, EP_GOAL_D2])                        # the ticks moved the agents


def test_planar_and_3d_give_the_same_record():
    (p, pd, _), (z, zd, _) = _staged(False)[0], _staged(True)[0]
    assert np.array_equal(_bits(p), _bits(z)) and np.array_equal(pd, zd)


@pytest.mark.parametrize("q", [1, 4, 9, 10, 12])
def test_a_scene_alone_gives_the_record_it_gives_inside_the_batch(q):
    for k, ((rec, done, _), (alone, alone_done, _)) in enumerate(zip(_staged(False), _staged(False, q))):
        _same_bits(alone[0], rec[q], f"stage {k}, scene {q}")
        assert alone_done[0] == done[q]


# ---- 2. the strict `<` of every rule, on the device --------------------------------------------------------------------------------

def test_edges_of_the_rules_on_the_device():
    tri = bare([[0, 0], [3, 4], [40, 40]], dynamic_obstacles=[ring([-5, 3], [[-4, 3], [-6, 3], [-6, 5]])])
    coincident = bare([[1, 1], [1, 1]], wp=[[1, 1], [9, 9]], dynamic_obstacles=[ring([1, 1], [[1, 1]])])
    goal = bare([[2, 1]], wp=[[5, 5]])
    away = ring([np.inf, np.inf], np.full((4, 2), np.inf))
    walls = dict(borders=[np.array([[0.0, 3.0], [0.0, 4.0]])], border_centers=np.array([[0.0, 3.5]]), border_lengths=np.array([1.0]),
                 static_obstacles=[ring([2, 0], [[2.0, 0.0], [3.0, 0.0]])])
    cases = [  # (scene, agent, (goal, ped, veh radius), max_steps, reason, done)
        (tri, 0, (0.0, 5.0, 5.0), 0, 0),
        (tri, 0, (0.0, JUST_ABOVE_5, 5.0), 0, REASON_PED_HIT),
        (tri, 0, (0.0, 5.0, JUST_ABOVE_5), 0, REASON_VEH_HIT),
        (tri, 0, (0.0, JUST_ABOVE_5, JUST_ABOVE_5), 1, REASON_PED_HIT + REASON_VEH_HIT + REASON_TIME_LIMIT),
        (coincident, 0, (0.0, 0.0, 0.0), 0, 0),
        (goal, 0, (5.0, 0.0, 0.0), 0, 0),
        (goal, 0, (JUST_ABOVE_5, 0.0, 0.0), 0, REASON_ARRIVED),
        (bare([[2.0e12, 0.0], [3, 4]]), 0, (1.0, 1.0, 1.0), 0, REASON_NOT_LIVE),
        (bare([[0.0, np.nan], [3, 4]]), 0, (1.0, 1.0, 1.0), 0, REASON_NOT_LIVE),
        (bare([[0.0, np.nan], [3, 4], [2.0e12, 4]]), 1, (0.0, 1e6, 0.0), 0, 0),          # ghosts are nobody's hit
        (bare([[0, 0], [0.1, 0]], wp=[[0, 0], [0, 0]]), -1, (5.0, 5.0, 5.0), 1, REASON_TIME_LIMIT),
        (bare([[0, 0], [0.1, 0]], wp=[[0, 0], [0, 0]]), -1, (5.0, 5.0, 5.0), 2, 0),
        (bare(np.zeros((0, 2))), -1, (5.0, 5.0, 5.0), 0, 0),
        (bare([[1, 2]]), 0, (1.0, 1e6, 1e6), 0, 0),                                            # N_b = 1, no geometry
        (bare([[1, 2]], dynamic_obstacles=[away]), 0, (0.0, 0.0, 1e6), 0, 0),
        (bare([[1, 2]], dynamic_obstacles=[away, ring([1, 4], [[1, 4], [2, 4]])]), 0, (0.0, 0.0, 1e6), 0, REASON_VEH_HIT),
        (bare([[0, 0]], **walls), 0, (0.0, 1e6, 1e6), 0, 0),
    ]
    scenes = [c[0] for c in cases]
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), 0.05, B=len(cases))
    try:
        b.upload(scenes)
        b.set_episodes([c[1] for c in cases], *([c[2][k] for c in cases] for k in range(3)), [c[3] for c in cases])
        b.end_step()
        rec, done = b.episodes()
        for q, (sc, agent, radii, ms, reason) in enumerate(cases):
            want, _ = episode_scene(sc, agent, radii, ms)
            _same_bits(rec[q], want, f"case {q}")
            assert rec[q, EP_REASON] == reason and done[q] == (reason != 0) and rec[q, EP_DONE] == float(reason != 0), f"case {q}"
        assert rec[0, EP_PED_D2] == 25.0 and rec[0, EP_VEH_D2] == 25.0 and rec[5, EP_GOAL_D2] == 25.0
        assert (rec[7, EP_GOAL_D2:] == INF).all() and (rec[8, EP_GOAL_D2:] == INF).all() and (rec[12, EP_GOAL_D2:] == INF).all()
        assert rec[9, EP_PED_D2] == INF and rec[13, EP_PED_D2] == INF and rec[14, EP_VEH_D2] == INF and rec[15, EP_VEH_D2] == 4.0
        assert rec[16, EP_WALL_D2] == 4.0 and rec[13, EP_WALL_D2] == INF
        # the second evaluation: prev carried over, the time limit of 2 reached, a dead agent's stored prev left alone (NaN -> +inf out)
        b.end_step()
        rec2, done2 = b.episodes()
        assert np.array_equal(rec2[:, EP_AGE], np.full(len(cases), 2, np.float32))
        assert rec2[11, EP_REASON] == REASON_TIME_LIMIT and done2[11]
        assert rec2[5, EP_PREV_GOAL_D2] == 25.0 and rec2[7, EP_PREV_GOAL_D2] == INF
    finally:
        b.close()


# ---- 3. an evaluation changes nothing a tick computes ------------------------------------------------------------------------------

def test_end_step_changes_nothing_a_tick_or_an_observation_computes():
    scenes = [_scenes()[q] for q in (3, 6, 9, 11)]

    def go(evaluate):
        b = _batch(scenes, episodes=evaluate)
        try:
            b.set_observation(4, 5.0)
            b.run(5)
            if evaluate:
                b.end_step()
            b.run(5)
            return b.state(), b.observations(), b.dynamic_obstacles(), b.waypoints()
        finally:
            b.close()

    (s0, o0, v0, w0), (s1, o1, v1, w1) = go(False), go(True)
    for q in range(len(scenes)):
        assert np.array_equal(s0[q][0], s1[q][0]) and np.array_equal(s0[q][1], s1[q][1]), q
        assert np.array_equal(_bits(o0[q]), _bits(o1[q])), q
        assert all(np.array_equal(a[1], c[1]) for a, c in zip(v0[q], v1[q])) and np.array_equal(w0[q][0], w1[q][0]), q


# ---- 4. the restart by device mask against the restart by host mask ----------------------------------------------------------------

def _full():
    """Four scenes (0, 5, 70, 300 rows) with modes, a spawn schedule and device vehicles on tracks (three scenes have vehicles)."""
    scenes, plans, scheds, tracks = R._made(False)
    b = SfmBatch([M._config(k) for k in range(len(R.SIZES))], list(R.DTS))
    try:
        b.upload(scenes, device_vehicles=True)
        b.set_vehicle_tracks(tracks)
        b.set_modes(plans, despawn_on_arrival=True, sim_time0=list(R.T0), arrive_thresholds=2.0, scenes=scenes)
        b.set_spawns(scheds)
    except Exception:
        b.close()
        raise
    return b


def _read_all(b):
    out = [{"loc": loc, "vel": vel, "wp": wp, "draws": d, "ctr": [c for c, _ in veh], "ring": [r for _, r in veh]}
           for (loc, vel), (wp, d), veh in zip(b.state(), b.waypoints(), b.dynamic_obstacles())]
    clocks = b.clocks()
    tick, present = b.vehicle_tracks()
    for k, ((m, t, c), (born, when)) in enumerate(zip(b.modes(), b.spawns())):
        out[k].update(mode=m, target=t, cursor=c, clock=clocks[k:k + 1], born=born, birth=when, present=present[k],
                      tick=np.array([tick]))
    return out


def _assert_batches_agree(a, c, what):
    for k, (u, v) in enumerate(zip(_read_all(a), _read_all(c))):
        R._assert_scene(u, v, f"{what}: scene {k}")


def _mask_tensor(mask, dtype=None):
    import torch
    return torch.tensor(np.asarray(mask, dtype=np.uint8), dtype=dtype or torch.uint8, device="cuda")


def test_restart_device_equals_restart_by_host_mask():
    mask = [0, 1, 0, 1]
    a, c, f = _full(), _full(), _full()
    try:
        for b in (a, c, f):
            b.run(2)
            b.snapshot()
            b.run(7)
        before = _read_all(a)
        a.restart_device(_mask_tensor(mask))
        c.restart(np.array(mask, dtype=bool))
        after = _read_all(a)
        for k in (0, 2):                                                # the scenes not chosen are not touched
            R._assert_scene(after[k], before[k], f"left alone: scene {k}")
        assert not R._same_array(after[3]["loc"], before[3]["loc"])
        for b in (a, c, f):
            b.run(7)
        _assert_batches_agree(a, c, "device mask against host mask")
        ra, rf = _read_all(a), _read_all(f)
        assert not R._same_array(ra[3]["loc"], rf[3]["loc"]) and R._same_array(ra[2]["loc"], rf[2]["loc"])    # the restart mattered
        assert a.vehicle_tracks()[0] == 16
    finally:
        for b in (a, c, f):
            b.close()


def test_restart_device_edge_masks_and_a_snapshot_after_it():
    import torch
    a, c = _full(), _full()
    try:
        for b in (a, c):
            b.run(3)
            b.snapshot()
            b.run(6)
        before = _read_all(a)
        a.restart_device(_mask_tensor([0, 0, 0, 0]))                    # nobody: nothing changes
        for k, (u, v) in enumerate(zip(_read_all(a), before)):
            R._assert_scene(u, v, f"all-zero mask: scene {k}")
        a.restart_device(_mask_tensor([1, 1, 1, 1], torch.bool))        # everybody: restart(None)
        c.restart()
        for b in (a, c):
            b.run(4)
        _assert_batches_agree(a, c, "all-ones mask against restart(None)")
        # any nonzero byte chooses; then a snapshot taken after a device restart (it must read the first ticks back from the
        # device), and a host restart from it
        a.restart_device(_mask_tensor([0, 7, 255, 0]))
        c.restart([1, 2])
        for b in (a, c):
            b.run(2)
            b.snapshot()
            b.run(5)
            b.restart([2, 3])
            b.run(4)
        _assert_batches_agree(a, c, "snapshot after a device restart, then a host restart")
        a.restart_device(_mask_tensor([0, 0, 1, 1], torch.int8))
        c.restart([2, 3])
        a.restart([1])                                                  # a host restart while the host's first ticks are stale
        c.restart([1])
        for b in (a, c):
            b.run(3)
        _assert_batches_agree(a, c, "host restart after a device restart")
    finally:
        a.close()
        c.close()


# ---- 5. the auto restart against a host-driven loop --------------------------------------------------------------------------------

def test_auto_restart_equals_a_host_driven_loop():
    """7 steps of run(2) + end_step(auto_restart=True) against run(2), end_step(), episodes(), restart(done): the records of every
    step (checked against the twin, whose episode state starts over at every restart -- so the age reads 0 after a restart by either
    mask) and the state at the end."""
    sizes = (5, 70, 40, 90, 3, 64, 257, 1)
    scenes = [G._scene(n, 6100 + q, dynamic=3 if q in (2, 3) else 0) for q, n in enumerate(sizes)]
    agents = _agents(sizes)
    B = len(sizes)
    settings = ([1.0] * B, [0.3] * B, [0.5] * B, [3 if q % 2 == 0 else 0 for q in range(B)])
    a, c = _batch(scenes, agents=agents, episodes=False), _batch(scenes, agents=agents, episodes=False)
    try:
        for b in (a, c):
            b.set_episodes(agents, *settings)
            b.run(1)
            b.snapshot()
        ages, prevs = [0] * B, [np.nan] * B
        restarts, reasons, was_done = 0, 0, np.zeros(B, bool)
        for step in range(7):
            a.run(2)
            a.end_step(auto_restart=True)
            c.run(2)
            c.end_step()
            rec_c, done = c.episodes()
            want = _twin_rows(c, scenes, agents, settings, ages, prevs)
            rec_a, done_a = a.episodes()                                # the terminal values, kept through the restart
            for q in range(B):
                _same_bits(rec_c[q], want[q], f"step {step}, scene {q}: host loop against the twin")
                _same_bits(rec_a[q], rec_c[q], f"step {step}, scene {q}: auto restart against the host loop")
            assert np.array_equal(done_a, done)
            if done.any():
                c.restart(done)
                restarts += int(done.sum())
                for q in np.flatnonzero(done):
                    ages[q], prevs[q] = 0, np.nan
            assert (rec_a[was_done, EP_AGE] == 1).all()                 # a restarted scene's age read 0 when this step began
            assert (rec_a[::2, EP_AGE] <= 3).all()                      # max_steps = 3 on the even scenes
            was_done = done
            reasons |= int(np.bitwise_or.reduce(rec_a[:, EP_REASON].astype(np.int64)))
        assert restarts >= 2 * (B // 2) and reasons & REASON_TIME_LIMIT    # no even scene outlasts 3 steps: each ends twice at least
        for q, ((la, va), (lc, vc)) in enumerate(zip(a.state(), c.state())):
            assert np.array_equal(la, lc) and np.array_equal(va, vc), f"scene {q}"
        for va, vc in zip(a.dynamic_obstacles(), c.dynamic_obstacles()):
            assert all(np.array_equal(p[1], r[1]) for p, r in zip(va, vc))
    finally:
        a.close()
        c.close()


# ---- 6. the device views -----------------------------------------------------------------------------------------------------------

def test_device_views_alias_the_buffers():
    import torch
    scenes = [_scenes()[q] for q in (3, 6, 11, 0)]
    a, c = _batch(scenes), _batch(scenes)
    try:
        for b in (a, c):
            b.set_stream(torch.cuda.current_stream().cuda_stream)
            b.snapshot()
            b.run(3)
            b.end_step()
        rec_t, done_t = a.episode_tensor(), a.done_tensor()
        assert rec_t.shape == (4, 8) and rec_t.dtype == torch.float32 and done_t.shape == (4,) and done_t.dtype == torch.uint8
        assert rec_t.data_ptr() == a.device_ptr(PTR_EPISODES)[0] and done_t.data_ptr() == a.device_ptr(PTR_DONE)[0]
        assert a.device_ptr(PTR_EPISODES)[1] == 4 * 8 * 4 and a.device_ptr(PTR_DONE)[1] == 4
        rec, done = a.episodes()
        assert np.array_equal(_bits(rec_t.cpu().numpy()), _bits(rec)) and np.array_equal(done_t.cpu().numpy() != 0, done)
        a.end_step()                                                    # the views follow the buffers
        torch.cuda.synchronize()
        assert np.array_equal(rec_t[:, EP_AGE].cpu().numpy(), np.full(4, 2, np.float32))
        for b in (a, c):                                                # a mask of the caller's making, written through the view
            b.done_tensor().copy_(_mask_tensor([1, 0, 1, 0]))
        assert np.array_equal(a.episodes()[1], [True, False, True, False])
        a.restart_device(a.done_tensor())
        c.restart_device()
        for b in (a, c):
            b.run(2)
        for q, ((la, va), (lc, vc)) in enumerate(zip(a.state(), c.state())):
            assert np.array_equal(la, lc) and np.array_equal(va, vc), f"scene {q}"
        with pytest.raises(ValueError, match="bool, uint8 or int8"):
            a.restart_device(torch.zeros(4, dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError, match="on the device"):
            a.restart_device(torch.zeros(4, dtype=torch.uint8))
        with pytest.raises(ValueError, match="contiguous elements"):
            a.restart_device(torch.zeros(5, dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError, match="contiguous"):
            a.restart_device(torch.zeros(8, dtype=torch.uint8, device="cuda")[::2])
        with pytest.raises(ValueError, match="torch tensor"):
            a.restart_device(np.zeros(4, np.uint8))
    finally:
        a.close()
        c.close()


# ---- 7. every refusal leaves the batch usable --------------------------------------------------------------------------------------

def test_refusals_leave_the_batch_usable():
    scenes = [_scenes()[q] for q in (3, 6, 11, 0)]                      # 3, 65, 40 (vehicles) and 0 rows
    agents, good = [0, 64, 20, -1], ([1.0] * 4, [0.3] * 4, [0.5] * 4, [0, 2, 0, 1])
    err = lambda b: b._lib.sfm_batch_last_error(b._b).decode()
    ip, fp = _lib.iptr, _lib.fptr
    ag = np.array(agents, np.int32)
    r = np.ones(4, np.float32)
    ms = np.zeros(4, np.int32)
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), 0.05, B=4)
    L = b._lib
    try:
        # before upload
        assert L.sfm_batch_set_episodes(b._b, ip(ag), fp(r), fp(r), fp(r), ip(ms)) == SFM_ERR_STATE and "sfm_batch_upload_state" in err(b)
        assert L.sfm_batch_end_step(b._b, 0) == SFM_ERR_STATE and "episodes are off" in err(b)
        assert L.sfm_batch_download_episodes(b._b, None, None) == SFM_ERR_STATE
        assert L.sfm_batch_restart_device(b._b, None) == SFM_ERR_STATE and "no snapshot" in err(b)
        assert L.sfm_batch_set_episodes(b._b, None, None, None, None, None) == 0                 # off is always fine
        with pytest.raises(SfmLibraryError, match="upload"):
            b.set_episodes(0)
        b.upload(scenes, device_vehicles=True)
        # episodes off
        with pytest.raises(SfmLibraryError, match="episodes are off"):
            b.end_step()
        with pytest.raises(SfmLibraryError, match="episodes are off"):
            b.episodes()
        with pytest.raises(SfmLibraryError, match="episodes are off"):
            b.episode_tensor()
        for which in (PTR_EPISODES, PTR_DONE):
            assert L.sfm_batch_device_ptr(b._b, which, None) is None and "episodes are off" in err(b)
        assert L.sfm_batch_device_ptr(b._b, 5, None) is None and "which" in err(b)
        # bad settings: nothing changes (episodes stay off)
        for bad in ([3, 0, 0, -1], [0, 65, 0, -1], [0, 0, 0, 0], [-2, 0, 0, -1]):
            assert L.sfm_batch_set_episodes(b._b, ip(np.array(bad, np.int32)), fp(r), fp(r), fp(r), ip(ms)) == SFM_ERR_INVALID
            assert "agent must be" in err(b)
        with pytest.raises(ValueError, match="is no row"):
            b.set_episodes([3, 0, 0, -1])
        for col in range(3):
            for val in (np.nan, -1.0, np.inf, 2.0e6):
                cols = [r.copy(), r.copy(), r.copy()]
                cols[col][2] = val
                assert L.sfm_batch_set_episodes(b._b, ip(ag), *(fp(x) for x in cols), ip(ms)) == SFM_ERR_INVALID
                assert f"scene 2: {('goal_radius', 'ped_radius', 'veh_radius')[col]} must be finite" in err(b)
        assert L.sfm_batch_set_episodes(b._b, ip(ag), fp(r), fp(r), fp(r), ip(np.array([0, 0, -1, 0], np.int32))) == SFM_ERR_INVALID
        assert "scene 2: max_steps" in err(b)
        for hole in range(4):
            args = [fp(r), fp(r), fp(r), ip(ms)]
            args[hole] = None
            assert L.sfm_batch_set_episodes(b._b, ip(ag), *args) == SFM_ERR_INVALID and "NULL" in err(b)
        assert L.sfm_batch_end_step(b._b, 0) == SFM_ERR_STATE and not b.has_episodes
        # on; no snapshot
        b.set_episodes(agents, *good)
        assert b.has_episodes
        assert L.sfm_batch_end_step(b._b, 2) == SFM_ERR_INVALID and "SFM_END_STEP_AUTO_RESTART" in err(b)
        with pytest.raises(SfmLibraryError, match="no snapshot"):
            b.end_step(auto_restart=True)
        assert not b.episodes()[0].any()                                # nothing was launched: the record is still zeros
        with pytest.raises(SfmLibraryError, match="no snapshot"):
            b.restart_device()
        b.end_step()
        rec, _ = b.episodes()
        assert np.array_equal(rec[:, EP_AGE], np.ones(4, np.float32))
        # a refused set_episodes keeps the episodes that are on, state included
        assert L.sfm_batch_set_episodes(b._b, ip(np.array([9, 0, 0, -1], np.int32)), fp(r), fp(r), fp(r), ip(ms)) == SFM_ERR_INVALID
        b.end_step()
        assert np.array_equal(b.episodes()[0][:, EP_AGE], np.full(4, 2, np.float32))
        # snapshot; a NULL mask
        b.snapshot()
        assert L.sfm_batch_restart_device(b._b, None) == SFM_ERR_INVALID and "d_mask is NULL" in err(b)
        b.run(2)
        b.end_step(auto_restart=True)                                   # scenes 1 (max_steps 2) and 3 (max_steps 1) are over
        rec, done = b.episodes()
        assert done[1] and done[3] and int(rec[1, EP_REASON]) & REASON_TIME_LIMIT
        b.end_step()
        assert np.array_equal(b.episodes()[0][[1, 3], EP_AGE], np.ones(2, np.float32))          # their age was 0
        # set_episodes keeps the snapshot and starts the episode state over; set_episodes(None) frees
        b.set_episodes(agents, *good)
        assert b.has_snapshot and not b.episodes()[0].any()
        b.end_step(auto_restart=True)
        assert np.array_equal(b.episodes()[0][:, EP_AGE], np.ones(4, np.float32))
        b.set_episodes(None)
        assert not b.has_episodes and b.has_snapshot
        for which in (PTR_EPISODES, PTR_DONE):
            assert L.sfm_batch_device_ptr(b._b, which, None) is None and "episodes are off" in err(b)
        with pytest.raises(SfmLibraryError, match="episodes are off"):
            b.end_step()
        b.restart()                                                     # a batch without episodes restarts as it did
        b.run(1)
        # upload drops the episodes
        b.set_episodes(agents, *good)
        b.upload(scenes, device_vehicles=True)
        assert not b.has_episodes
        with pytest.raises(SfmLibraryError, match="episodes are off"):
            b.end_step()
        b.set_episodes(agents, *good)
        b.run(1)
        b.end_step()
        assert np.array_equal(b.episodes()[0][:, EP_AGE], np.ones(4, np.float32))
    finally:
        b.close()


def test_the_device_loop_example_runs():
    spec = importlib.util.spec_from_file_location("batch_rl_loop_device", os.path.join(ROOT, "examples", "batch_rl_loop_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    episodes, arrivals = ex.run(B=8, steps=6, repeat=2, max_age=3, quiet=True)
    assert episodes >= 16 and 0 <= arrivals <= episodes                # max_age = 3: no episode outlasts 3 steps, so each scene ends twice at least
