"""GPU tests of the batch's row episodes and row respawns (sfm_batch_set_row_episodes, sfm_batch_end_row_step,
sfm_batch_respawn_rows_device; SfmBatch.set_row_episodes / end_row_step / respawn_rows_device).

The oracles are the NumPy twins ``episode.row_episode_scene`` and ``reset.respawn_rows_scene`` (pinned on the CPU in
tests/test_batch_row_episodes_host.py), the scene episodes of ``end_step`` where a scene has one agent, and the library's own guarantee
that a scene's result does not depend on the rest of the batch.  Every comparison is bitwise.  The crowd is the mixed batch of
tests/_row_episode_cases.py: twelve scenes of 0 .. 1 024 rows whose agent sets run the kernel with every value of its split.
Run on the MI355X box with  python -m pytest tests -m gpu."""
from functools import lru_cache

import numpy as np
import pytest

import _lifecycle_cases as LC
import _row_episode_cases as RC
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd._lib import SfmLibraryError, fptr, iptr, u8ptr
from carla_social_force_model_amd.batch import (EPISODE_WIDTH, PTR_ROW_DONE, PTR_ROW_EPISODES, PTR_ROW_RESETS, SfmBatch)
from carla_social_force_model_amd.config import default_sfm_config

pytestmark = pytest.mark.gpu

ALL = tuple(range(RC.B))
SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3
K0, K1 = 2, 3                    # ticks before the snapshot, ticks between the snapshot and a respawn


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32)).view(np.uint32)


def _same(u, v):
    """Bitwise, with NaN equal to NaN."""
    u, v = np.asarray(u), np.asarray(v)
    if u.shape != v.shape:
        return False
    if u.dtype.kind == "f" or v.dtype.kind == "f":
        u, v = u.astype(np.float32), v.astype(np.float32)
        nu, nv = np.isnan(u), np.isnan(v)
        return bool(np.array_equal(nu, nv) and np.array_equal(u[~nu].view(np.uint32), v[~nv].view(np.uint32)))
    return bool(np.array_equal(u, v))


@lru_cache(maxsize=None)
def _scenes3():
    """The planar scenes with heights: x, y are the planar batch's bit for bit."""
    out = []
    for k, sc in enumerate(RC.scenes()):
        rng = np.random.default_rng(9900 + k)
        sc = dict(sc)
        loc, vel = sc["loc"].copy(), sc["vel"].copy()
        loc[:, 2] = np.float32(rng.uniform(0.0, 1.5, loc.shape[0]))
        vel[:, 2] = np.float32(rng.normal(0.0, 0.05, loc.shape[0]))
        sc["loc"], sc["vel"] = loc, vel
        out.append(sc)
    return out


@lru_cache(maxsize=None)
def _tracks():
    return [scenarios.make_track_plan(sc, 9950 + k, 40, dt=RC.DTS[k]) if sc["dynamic_obstacles"] else None for k, sc in enumerate(RC.scenes())]


def _build(which=ALL, z3=False, episodes=True, noise=None, tracks=False):
    src = _scenes3() if z3 else RC.scenes()
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), [RC.DTS[k] for k in which])
    try:
        b.upload([src[k] for k in which], planar=False if z3 else None, device_vehicles=True)
        if tracks:
            b.set_vehicle_tracks([_tracks()[k] for k in which])
        if episodes:
            b.set_row_episodes(**RC.episode_args(which))
        if noise is not None:
            b.set_restart_noise(**RC.noise_args(which, **noise))
    except Exception:
        b.close()
        raise
    return b


def _now(b):
    """(state, waypoints, vehicles) per scene, as the twins take them."""
    return [(st, wp, veh) for st, (wp, _), veh in zip(b.state(), b.waypoints(), b.dynamic_obstacles())]


def _split(b, a):
    so = b.scene_off
    return [a[so[k]:so[k + 1]] for k in range(b.B)]


def _evaluate(b, which, ages, prevs):
    """One end_row_step against the twin; returns the new (ages, prevs) per scene and what the device left, per scene."""
    now = _now(b)
    b.end_row_step()
    got = [_split(b, a) for a in b.row_episodes()]
    for q, k in enumerate(which):
        st, wp, veh = now[q]
        rec, done, age, prev = RC.twin(k, st, wp, veh, ages[q], prevs[q])
        ag = RC.agents()[k]
        assert _same(got[0][q][ag], rec[ag]), f"scene {k}: record"
        assert np.array_equal(got[1][q][ag], done[ag]), f"scene {k}: row_done"
        assert np.array_equal(got[2][q], age), f"scene {k}: row_age"
        assert _same(got[3][q], prev), f"scene {k}: row_prev_goal_d2"
        ages[q], prevs[q] = age, prev
    return got


# ---- G1 ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ticks", [0, 1, 5])
def test_records_and_row_state_equal_the_twin(ticks):
    import torch
    b = _build()
    try:
        rec_t, done_t = b.row_episode_tensor(), b.row_done_tensor()
        rec_t.fill_(float("nan"))
        done_t.fill_(0xFF)
        torch.cuda.synchronize()
        ages, prevs = [None] * b.B, [None] * b.B
        reasons = set()
        for _ in range(3):
            if ticks:
                b.run(ticks)
            got = _evaluate(b, ALL, ages, prevs)
            reasons |= set(np.concatenate(got[0])[np.concatenate(RC.agents()), 1].astype(int).tolist())
        torch.cuda.synchronize()
        other = ~np.concatenate(RC.agents())
        assert other.any() and np.isnan(rec_t.cpu().numpy()[other]).all() and (done_t.cpu().numpy()[other] == 0xFF).all()
        assert all(any(r & bit for r in reasons) for bit in (1, 2, 4, 16)), reasons      # arrivals, time limits, hits, a row that is not live
    finally:
        b.close()


# ---- G2 ---------------------------------------------------------------------------------------------------------------------------------

def test_one_agent_per_scene_equals_end_step():
    agent = [-1 if n == 0 else min(n - 1, 5 + 3 * k) for k, n in enumerate(RC.SIZES)]
    flags = [np.arange(n) == a for n, a in zip(RC.SIZES, agent)]
    b = _build(episodes=False)
    try:
        kw = dict(goal_radius=list(RC.GOAL_R), ped_radius=list(RC.PED_R), veh_radius=list(RC.VEH_R), max_steps=list(RC.MAX_STEPS))
        b.set_episodes(agent, **kw)
        b.set_row_episodes(flags, **kw)
        rows = [int(b.scene_off[k]) + a for k, a in enumerate(agent) if a >= 0]
        for _ in range(3):
            b.run(2)
            b.end_step()
            b.end_row_step()
            rec, done = b.episodes()
            rrec, rdone, _, _ = b.row_episodes()
            keep = [k for k, a in enumerate(agent) if a >= 0]
            assert _same(rrec[rows], rec[keep]) and np.array_equal(rdone[rows], done[keep])
            assert b.row_episode_tensor()[rows].cpu().numpy().tobytes() == b.episode_tensor()[keep].cpu().numpy().tobytes()
    finally:
        b.close()


# ---- G3 ---------------------------------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _mixed():
    """The mixed batch after one tick and two evaluations one tick apart: what every scene alone must reproduce."""
    b = _build()
    try:
        out = []
        for _ in range(2):
            b.run(1)
            b.end_row_step()
            out.append([_split(b, a) for a in b.row_episodes()])
        return out
    finally:
        b.close()


@pytest.mark.parametrize("k", ALL)
def test_a_scene_alone_equals_the_scene_in_the_mixed_batch(k):
    b = _build((k,))
    try:
        for want in _mixed():
            b.run(1)
            b.end_row_step()
            for got, w in zip(b.row_episodes(), want):
                assert _same(got, w[k])
    finally:
        b.close()


def test_a_3d_batch_gives_the_planar_record():
    p, z = _build(), _build(z3=True)
    try:
        assert p.planar and not z.planar
        p.end_row_step()
        z.end_row_step()
        for u, v in zip(p.row_episodes(), z.row_episodes()):
            assert _same(u, v)
    finally:
        p.close()
        z.close()


def test_row_episodes_change_nothing_else():
    kw = dict(goal_radius=3.0, ped_radius=0.9, veh_radius=1.0, max_steps=4)
    out = []
    for rows in (False, True):
        b = _build(episodes=rows)
        try:
            b.set_observation(4, 8.0)
            b.set_episodes([-1 if n == 0 else 0 for n in RC.SIZES], **kw)
            got = []
            for _ in range(3):
                b.run(3)
                if rows:
                    b.end_row_step()
                b.observe()
                b.end_step()
                if rows:
                    b.end_row_step()
                got.append((b.state_arrays(), b.observations(), b.episodes(), b.waypoints(), b.dynamic_obstacles()))
            out.append(got)
        finally:
            b.close()
    for (s0, o0, e0, w0, d0), (s1, o1, e1, w1, d1) in zip(*out):
        assert all(_same(u, v) for u, v in zip(s0, s1)) and all(_same(u, v) for u, v in zip(e0, e1))
        assert all(_same(u, v) for u, v in zip(o0, o1))
        assert all(_same(u[0], v[0]) and _same(u[1], v[1]) for u, v in zip(w0, w1))
        assert all(len(u) == len(v) and all(_same(c, e) and _same(r, s) for (c, r), (e, s) in zip(u, v)) for u, v in zip(d0, d1))


# ---- G4 ---------------------------------------------------------------------------------------------------------------------------------

def _read(b, modes=False, tracks=False):
    """Everything readable, per scene."""
    out = [{"loc": loc, "vel": vel, "wp": wp, "draws": d, "ctr": [c for c, _ in veh], "ring": [r for _, r in veh]}
           for (loc, vel), (wp, d), veh in zip(b.state(), b.waypoints(), b.dynamic_obstacles())]
    if modes:
        clocks = b.clocks()
        for k, (m, t, c) in enumerate(b.modes()):
            out[k].update(mode=m, target=t, cursor=c, clock=clocks[k:k + 1])
    if tracks:
        for k, p in enumerate(b.vehicle_tracks()[1]):
            out[k].update(present=np.asarray(p))
    return out


PER_ROW = ("loc", "vel", "wp", "draws", "mode", "target", "cursor")


def _assert_respawned(after, before, snap, chosen, what):
    """Chosen rows hold the snapshot's entries of the per-row arrays, everything else is as before."""
    for k, (a, b0, s) in enumerate(zip(after, before, snap)):
        ch = np.asarray(chosen[k], bool)
        for name, u in a.items():
            if isinstance(u, list):
                assert len(u) == len(b0[name]) and all(_same(p, q) for p, q in zip(u, b0[name])), f"{what}: scene {k}: {name}"
            elif name in PER_ROW:
                assert _same(u[ch], s[name][ch]), f"{what}: scene {k}: chosen rows' {name}"
                assert _same(u[~ch], b0[name][~ch]), f"{what}: scene {k}: other rows' {name}"
            else:
                assert _same(u, b0[name]), f"{what}: scene {k}: {name}"


def _masks(which):
    none = [np.zeros(n, bool) for n in RC.SIZES]
    one = [m.copy() for m in none]
    one[7][130] = True
    scene = [m.copy() for m in none]
    scene[8][:] = True
    third = [np.arange(n) % 3 == 1 for n in RC.SIZES]
    return {"none": none, "one": one, "scene": scene, "third": third}[which]


def _device_mask(chosen):
    import torch
    return torch.as_tensor(np.concatenate([np.asarray(c, bool) for c in chosen]), device="cuda")


@pytest.mark.parametrize("which,z3", [("none", False), ("one", False), ("scene", False), ("third", False), ("third", True)])
def test_respawn_without_noise_copies_the_chosen_rows_only(which, z3):
    import torch
    chosen = _masks(which)
    b = _build(z3=z3, tracks=True)
    try:
        b.run(K0)
        b.snapshot()
        snap, snap_now = _read(b, tracks=True), _now(b)
        b.run(K1)
        b.end_row_step()
        b.end_row_step()
        before, now = _read(b, tracks=True), _now(b)
        ages0 = _split(b, b.row_episodes()[2])
        mask = _device_mask(chosen)
        b.respawn_rows_device(mask)
        after = _read(b, tracks=True)
        torch.cuda.synchronize()
        _assert_respawned(after, before, snap, chosen, which)
        for k in ALL:                                                   # ... and the twin says the same
            loc, vel, wp, _, fb = RC.respawn_twin(k, chosen[k], (snap_now[k][0], snap_now[k][1]), now[k], noise=False)
            assert fb is None and _same(after[k]["loc"], loc) and _same(after[k]["vel"], vel) and _same(after[k]["wp"], wp)
        if z3:
            assert any((after[k]["loc"][chosen[k], 2] != before[k]["loc"][chosen[k], 2]).any() for k in ALL)     # {z, vz} came back too
        _, _, ages, prevs = b.row_episodes()
        for k, (age, prev) in enumerate(zip(_split(b, ages), _split(b, prevs))):
            ag, ch = RC.agents()[k], chosen[k]
            assert not age[ch].any() and np.isnan(prev[ch]).all()
            assert np.array_equal(age[~ch], ages0[k][~ch]) and (age[ag & ~ch] == 2).all()
        if which != "none":
            assert any((after[k]["loc"] != before[k]["loc"]).any() for k in ALL)
    finally:
        b.close()


def test_respawn_with_modes_brings_a_despawned_row_back():
    import torch
    which = (10, 11)
    scenes = [RC.scenes()[k] for k in which]
    plans = [scenarios.make_mode_plan(sc, 9960 + q, queue_len=1)[0] for q, sc in enumerate(scenes)]
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), [RC.DTS[k] for k in which])
    try:
        b.upload(scenes, device_vehicles=True)
        b.set_modes(plans, despawn_on_arrival=True, sim_time0=4.5, arrive_thresholds=6.0, scenes=scenes)
        b.set_row_episodes(True, goal_radius=1.0, max_steps=0)
        b.snapshot()
        snap = _read(b, modes=True)
        b.run(60)
        before = _read(b, modes=True)
        gone = [r["mode"] == 255 for r in before]
        assert sum(int(g.sum()) for g in gone) > 0 and not any((r["mode"] == 255).any() for r in snap)
        chosen = [g | (np.arange(g.shape[0]) % 4 == 0) for g in gone]
        b.respawn_rows_device(_device_mask(chosen))
        after = _read(b, modes=True)
        torch.cuda.synchronize()
        _assert_respawned(after, before, snap, chosen, "modes")
        assert not any((r["mode"][c] == 255).any() for r, c in zip(after, chosen))
        assert all((np.abs(r["loc"][c, :2]) < 1e12).all() for r, c in zip(after, chosen))                # live again
        b.run(2)                                                        # ... and the scene goes on with them
    finally:
        b.close()


@pytest.mark.parametrize("path", ["host", "device", "end_step"])
def test_a_scene_restart_starts_the_row_episodes_of_the_restarted_scenes_over(path):
    import torch
    restarted = np.zeros(RC.B, bool)
    restarted[[2, 6, 9, 10]] = True
    b = _build()
    try:
        if path == "end_step":
            b.set_episodes([-1 if n == 0 else 0 for n in RC.SIZES], max_steps=[1 if r else 0 for r in restarted])
        b.snapshot()
        b.run(1)
        b.end_row_step()
        b.end_row_step()
        _, _, ages0, prevs0 = b.row_episodes()
        if path == "host":
            b.restart(restarted)
        elif path == "device":
            b.restart_device(torch.as_tensor(restarted, device="cuda"))
        else:
            b.end_step(auto_restart=True)
            assert np.array_equal(b.episodes()[1], restarted)
        _, _, ages, prevs = b.row_episodes()
        for k, (a0, a1, p0, p1) in enumerate(zip(_split(b, ages0), _split(b, ages), _split(b, prevs0), _split(b, prevs))):
            if restarted[k]:
                assert (a0[RC.agents()[k]] == 2).all() and not a1.any() and np.isnan(p1).all()
            else:
                assert np.array_equal(a0, a1) and _same(p0, p1)
    finally:
        b.close()


# ---- G5 ---------------------------------------------------------------------------------------------------------------------------------

def test_three_noisy_respawns_equal_the_twin():
    import torch
    b = _build(noise={})
    try:
        b.run(K0)
        b.snapshot()
        snap = _now(b)
        resets = [np.zeros(n, np.uint32) for n in RC.SIZES]
        fallbacks = np.zeros(RC.B, np.uint32)
        seen = {"fallback": 0, "late": 0, "moved": 0}
        for step in range(3):
            b.run(2)
            now, draws0 = _now(b), [d for _, d in b.waypoints()]
            chosen = RC.chosen(step)
            b.respawn_rows_device(_device_mask(chosen))
            after = _now(b)
            torch.cuda.synchronize()
            got_resets, got_fb = b.row_respawns()
            for k in ALL:
                loc, vel, wp, resets[k], fb, info = RC.respawn_twin(k, chosen[k], (snap[k][0], snap[k][1]), now[k], row_resets=resets[k], detail=True)
                assert _same(after[k][0][0], loc) and _same(after[k][0][1], vel) and _same(after[k][1], wp), f"respawn {step}, scene {k}"
                if fb is not None:
                    fallbacks[k] = fb
                    seen["fallback"] += fb
                    seen["late"] += int((info["round"] > 0).sum())
                    seen["moved"] += int((info["round"] >= 0).sum())
            assert np.array_equal(got_resets, np.concatenate(resets)) and np.array_equal(got_fb, fallbacks), f"respawn {step}: counters"
            assert np.array_equal(b.restart_noise()[0], np.zeros(RC.B, np.uint32))                      # the scenes' own counters stay
        assert seen["moved"] > 100 and seen["late"] > 0 and seen["fallback"] > 0      # (nonzero fallback counts were compared)
    finally:
        b.close()


def _after_done_respawn(how):
    import torch
    b = _build(noise={})
    try:
        b.run(K0)
        b.snapshot()
        b.run(K1)
        if how == "auto":
            b.end_row_step(auto_respawn=True)
        else:
            b.end_row_step()
            done = b.row_done_tensor()
            assert int(done.sum()) > 10
            b.respawn_rows_device(None if how == "none" else done.clone().bool())
        out = (b.state_arrays(), b.waypoints(), b.row_respawns(), b.row_episodes())
        torch.cuda.synchronize()
        return out
    finally:
        b.close()


def test_row_done_a_torch_mask_and_the_auto_respawn_give_the_same():
    a, t, auto = (_after_done_respawn(how) for how in ("none", "torch", "auto"))
    for other in (t, auto):
        assert all(_same(u, v) for u, v in zip(a[0], other[0]))
        assert all(_same(u[0], v[0]) and _same(u[1], v[1]) for u, v in zip(a[1], other[1]))
        assert all(_same(u, v) for u, v in zip(a[2], other[2])) and all(_same(u, v) for u, v in zip(a[3], other[3]))
    rec, done, ages, _ = a[3]
    assert done.any() and rec[done, 0].all() and not ages[done].any()                                    # terminal values stay, the age starts over
    assert a[2][0].sum() == done.sum()


def test_the_property_holds_on_the_device_output():
    import torch
    which = RC.PROPERTY_SCENES
    b = _build(which, noise=RC.PROPERTY_GAPS)
    try:
        b.snapshot()
        b.run(K1)
        chosen = [RC.chosen(0)[k] for k in which]
        b.respawn_rows_device(_device_mask(chosen))
        after = _now(b)
        torch.cuda.synchronize()
        resets, fb = b.row_respawns()
        assert not fb.any() and np.array_equal(resets, np.concatenate(chosen).astype(np.uint32))
        pos = RC.boxes()[0]
        for q, k in enumerate(which):
            loc = after[q][0][0]
            live = (np.abs(loc[:, :2]) < 1e12).all(axis=1)
            moved = np.flatnonzero(chosen[q] & live & (pos[k] != 0).any(axis=1))
            dp, dq = RC.min_true_distances(loc[:, :2], moved, live, RC.scene_points(k, after[q][2]))
            assert len(moved) and (dp >= RC.PROPERTY_GAPS["min_gap"] * RC.GAP_SLACK).all() and (dq >= RC.PROPERTY_GAPS["point_gap"] * RC.GAP_SLACK).all()
    finally:
        b.close()


# ---- G6 ---------------------------------------------------------------------------------------------------------------------------------

def test_views_alias_the_buffers():
    import torch
    b = _build(noise={})
    try:
        n = int(b.scene_off[-1])
        rec_t, done_t = b.row_episode_tensor(), b.row_done_tensor()
        assert tuple(rec_t.shape) == (n, EPISODE_WIDTH) and rec_t.dtype == torch.float32
        assert tuple(done_t.shape) == (n,) and done_t.dtype == torch.uint8
        assert b.device_ptr(PTR_ROW_EPISODES) == (rec_t.data_ptr(), 32 * n) and b.device_ptr(PTR_ROW_DONE) == (done_t.data_ptr(), n)
        assert b.device_ptr(PTR_ROW_RESETS)[1] == 4 * n
        b.run(1)
        b.end_row_step()
        rec, done, _, _ = b.row_episodes()
        assert _same(rec_t.cpu().numpy(), rec) and np.array_equal(done_t.cpu().numpy().astype(bool), done) and done.any()
        b.set_row_episodes(None)
        assert not b.has_row_episodes
        with pytest.raises(SfmLibraryError, match="row episodes are off"):
            b.row_episode_tensor()
    finally:
        b.close()


def _everything(b):
    out = [b.state_arrays(), b.waypoints()]
    if b.has_row_episodes:
        out.append(b.row_episodes())
    return out


def _unchanged(u, v):
    return repr([[np.asarray(x).tobytes() for x in (e if isinstance(e, (tuple, list)) else [e])] for part in u for e in part]) == \
           repr([[np.asarray(x).tobytes() for x in (e if isinstance(e, (tuple, list)) else [e])] for part in v for e in part])


def test_refusals_change_nothing():
    L = None
    fresh = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), [0.05])
    try:
        L = fresh._lib
        one, r, ms = np.ones(1, np.uint8), np.ones(1, np.float32), np.zeros(1, np.int32)
        assert L.sfm_batch_set_row_episodes(fresh._b, u8ptr(one), fptr(r), fptr(r), fptr(r), iptr(ms)) == SFM_ERR_STATE     # before upload
        with pytest.raises(SfmLibraryError):
            fresh.set_row_episodes(True)
    finally:
        fresh.close()
    b = _build()
    try:
        b.run(1)
        b.end_row_step()
        n = int(b.scene_off[-1])
        held = _everything(b)
        ag = np.ones(n, np.uint8)
        good, ms = np.ones(b.B, np.float32), np.zeros(b.B, np.int32)
        for bad in (-1.0, np.nan, np.inf, 2.0e6):                       # a bad radius
            r = good.copy()
            r[3] = bad
            assert L.sfm_batch_set_row_episodes(b._b, u8ptr(ag), fptr(good), fptr(r), fptr(good), iptr(ms)) == SFM_ERR_INVALID
            with pytest.raises(ValueError):
                b.set_row_episodes(True, ped_radius=[bad if k == 3 else 1.0 for k in ALL])
        neg = ms.copy()
        neg[2] = -1
        assert L.sfm_batch_set_row_episodes(b._b, u8ptr(ag), fptr(good), fptr(good), fptr(good), iptr(neg)) == SFM_ERR_INVALID
        with pytest.raises(ValueError, match="one value per row"):     # a bad agents length (Python)
            b.set_row_episodes(np.ones(n + 1, bool))
        assert b.has_row_episodes and _unchanged(held, _everything(b))
        assert L.sfm_batch_respawn_rows_device(b._b, None) == SFM_ERR_STATE                              # no snapshot
        assert L.sfm_batch_end_row_step(b._b, 1) == SFM_ERR_STATE
        assert L.sfm_batch_end_row_step(b._b, 2) == SFM_ERR_INVALID
        with pytest.raises(SfmLibraryError, match="no snapshot"):
            b.respawn_rows_device()
        assert _unchanged(held, _everything(b))
        b.snapshot()
        b.set_row_episodes(None)
        assert L.sfm_batch_respawn_rows_device(b._b, None) == SFM_ERR_INVALID                            # a NULL mask while row episodes are off
        assert L.sfm_batch_end_row_step(b._b, 0) == SFM_ERR_STATE
        for which in (PTR_ROW_EPISODES, PTR_ROW_DONE, PTR_ROW_RESETS):                                   # the new ids while their feature is off
            assert not L.sfm_batch_device_ptr(b._b, which, None)
            with pytest.raises(SfmLibraryError, match="which must be"):
                b.device_ptr(which)
        with pytest.raises(SfmLibraryError):
            b.row_respawns()
        assert _unchanged(held[:2], _everything(b))
        b.set_row_episodes(**RC.episode_args())                         # upload drops the row episodes
        b.upload([RC.scenes()[k] for k in ALL], device_vehicles=True)
        assert not b.has_row_episodes and L.sfm_batch_end_row_step(b._b, 0) == SFM_ERR_STATE
    finally:
        b.close()
    for setup, message in (("spawns", "spawn schedule"), ("policy", "routes are set")):      # a spawn schedule; routes
        s = SfmBatch(LC.configs(), list(LC.DTS))
        try:
            c = LC.crowd("policy", "A")
            LC.set_everything(s, c)
            if setup == "spawns":
                s.set_routes(None, None, None)
                s.set_spawns(c["scheds"])
            s.snapshot()
            s.set_row_episodes(True)
            held = _everything(s)
            assert L.sfm_batch_respawn_rows_device(s._b, None) == SFM_ERR_STATE and L.sfm_batch_end_row_step(s._b, 1) == SFM_ERR_STATE
            with pytest.raises(SfmLibraryError, match=message):
                s.respawn_rows_device()
            with pytest.raises(SfmLibraryError, match=message):
                s.end_row_step(auto_respawn=True)
            assert _unchanged(held, _everything(s))
        finally:
            s.close()
