"""GPU tests of the batch's vehicle episodes and vehicle respawns (sfm_batch_set_vehicle_episodes, sfm_batch_end_vehicle_step,
sfm_batch_respawn_vehicles_device; SfmBatch.set_vehicle_episodes / end_vehicle_step / respawn_vehicles_device).

The oracles are the NumPy twins ``episode.vehicle_episode_scene`` and ``scenarios.respawn_vehicles_scene`` (pinned on the CPU in
tests/test_batch_vehicle_episodes_host.py) and the library's own guarantee that a scene's result does not depend on the rest of the
batch.  Every comparison is bitwise.  The scenes are the mixed batch of tests/_vehicle_episode_cases.py.  The per-vehicle episode
state has no download of its own: the age is slot 2 of the record, and the stored prev_goal_d2 shows in slot 4 of the NEXT
evaluation, which is how the tests read both.
Run on the MI355X box with  python -m pytest tests -m gpu."""
from functools import lru_cache

import numpy as np
import pytest

import _vehicle_episode_cases as VC
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd._lib import SfmLibraryError, fptr, iptr, u8ptr
from carla_social_force_model_amd.batch import (EPISODE_WIDTH, PTR_VEHICLE_DONE, PTR_VEHICLE_EPISODES, PTR_VEHICLE_SCENE_DONE, SfmBatch)
from carla_social_force_model_amd.config import default_sfm_config

pytestmark = pytest.mark.gpu

ALL = tuple(range(VC.B))
WITH_VEHICLES = tuple(k for k in ALL if VC.VEHICLES[k])
SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3
TURN = 0.03


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
    for k, sc in enumerate(VC.scenes()):
        rng = np.random.default_rng(9400 + k)
        sc = dict(sc)
        loc, vel = sc["loc"].copy(), sc["vel"].copy()
        loc[:, 2] = np.float32(rng.uniform(0.0, 1.5, loc.shape[0]))
        vel[:, 2] = np.float32(rng.normal(0.0, 0.05, loc.shape[0]))
        sc["loc"], sc["vel"] = loc, vel
        out.append(sc)
    return out


def _driving(which, tracks):
    """Agents that are not tracked are unicycles that turn a little; the others run free."""
    kinds, cmds = [], []
    for k in which:
        kd = np.where(VC.agents()[k], 2, 0).astype(np.uint8)
        if tracks and k in VC.ABSENT:
            kd[VC.ABSENT[k]] = 0
        kinds.append(kd)
        cmds.append(np.tile(np.float32([2.0, np.cos(TURN), np.sin(TURN)]), (VC.VEHICLES[k], 1)))
    return kinds, cmds


def _paths(which):
    """Every odd vehicle follows a path straight ahead, a point per metre: the cursor moves within the first ticks."""
    out = []
    for k in which:
        sc = VC.scenes()[k]
        per = []
        for v, (c, _) in enumerate(sc["dynamic_obstacles"]):
            h = np.asarray(sc["dynamic_heading"][v], dtype=np.float64)
            per.append(c + np.arange(1.0, 31.0)[:, None] * h if v % 2 else None)
        out.append(per)
    return out


def _build(which=ALL, z3=False, episodes=True, tracks=True, autopilot=False):
    src = _scenes3() if z3 else VC.scenes()
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), [VC.DTS[k] for k in which])
    try:
        b.upload([src[k] for k in which], planar=False if z3 else None)
        b.set_dynamic_boxes(VC.boxes(which))
        if tracks:
            b.set_vehicle_tracks(VC.tracks(which))
        b.set_vehicle_driving(*_driving(which, tracks))
        if autopilot:
            b.set_vehicle_autopilot(_paths(which))
        if episodes:
            b.set_vehicle_episodes(**VC.episode_args(which))
    except Exception:
        b.close()
        raise
    return b


def _now(b):
    """(state, vehicles, headings) per scene, as the twin takes them."""
    return [(st, veh, drv[2]) for st, veh, drv in zip(b.state(), b.dynamic_obstacles(), b.vehicle_driving())]


def _split(b, a):
    io = b._dyn[0]
    return [a[io[k]:io[k + 1]] for k in range(b.B)]


def _evaluate(b, which, ages, prevs, **flags):
    """One end_vehicle_step against the twin; keeps (ages, prevs) per scene; returns the records per scene."""
    now = _now(b)
    b.end_vehicle_step(**flags)
    rec, done, sd = b.vehicle_episodes()
    rec, done = _split(b, rec), _split(b, done)
    for q, k in enumerate(which):
        st, veh, h = now[q]
        want, wdone, wsd, age, prev = VC.twin(k, st, veh, h, ages[q], prevs[q])
        ag = VC.agents()[k]
        assert _same(rec[q][ag], want[ag]), f"scene {k}: record"
        assert np.array_equal(done[q][ag], wdone[ag]), f"scene {k}: vehicle_done"
        if ag.any():
            assert bool(sd[q]) == wsd, f"scene {k}: vehicle_scene_done"
        ages[q], prevs[q] = age, prev
    return rec


# ---- G1 ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ticks", [0, 1, 5])
def test_records_masks_and_state_equal_the_twin(ticks):
    import torch
    b = _build()
    try:
        rec_t, done_t, sd_t = b.vehicle_episode_tensor(), b.vehicle_done_tensor(), b.vehicle_scene_done_tensor()
        rec_t.fill_(float("nan"))
        done_t.fill_(0xFF)
        sd_t.fill_(0xFF)
        torch.cuda.synchronize()
        ages, prevs = [None] * b.B, [None] * b.B
        reasons = 0
        for _ in range(3):                                              # (the second and third evaluation read the state the first left)
            if ticks:
                b.run(ticks)
            got = _evaluate(b, ALL, ages, prevs)
            for r in np.concatenate(got)[np.concatenate(VC.agents()), 1]:
                reasons |= int(r)
        torch.cuda.synchronize()
        other = ~np.concatenate(VC.agents())
        assert other.any() and np.isnan(rec_t.cpu().numpy()[other]).all() and (done_t.cpu().numpy()[other] == 0xFF).all()
        idle = np.array([not a.any() for a in VC.agents()])             # scenes without agent vehicles are never written
        assert idle.any() and (sd_t.cpu().numpy()[idle] == 0xFF).all() and (sd_t.cpu().numpy()[~idle] <= 1).all()
        assert reasons & 2 and reasons & 16, reasons
        if ticks == 0:
            assert reasons == 1 | 2 | 4 | 8 | 16 | 32, reasons          # every reason, as the host test of the same scenes found
        up = _split(b, b.vehicle_episodes()[0])[VC.UP_SCENE][VC.UP_VEHICLE]
        assert np.isinf(up[6]) and up[6] > 0                            # the absent ring beside the heading (0, 1): +inf, not a contact
    finally:
        b.close()


# ---- G2 ---------------------------------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _mixed():
    """The mixed batch after one tick and two evaluations one tick apart: what every scene alone must reproduce."""
    b = _build()
    try:
        out = []
        for _ in range(2):
            b.run(1)
            b.end_vehicle_step()
            rec, done, sd = b.vehicle_episodes()
            out.append((_split(b, rec), _split(b, done), sd))
        return out
    finally:
        b.close()


@pytest.mark.parametrize("k", WITH_VEHICLES)       # (a batch without any vehicle has no device-side vehicles to set episodes for)
def test_a_scene_alone_equals_the_scene_in_the_mixed_batch(k):
    b = _build((k,))
    try:
        for rec, done, sd in _mixed():
            b.run(1)
            b.end_vehicle_step()
            r, d, s = b.vehicle_episodes()
            assert _same(r, rec[k]) and np.array_equal(d, done[k]) and bool(s[0]) == bool(sd[k])
    finally:
        b.close()


def test_a_3d_batch_gives_the_planar_record():
    p, z = _build(), _build(z3=True)
    try:
        assert p.planar and not z.planar
        for _ in range(2):                                              # (no tick in between: heights change how a 3-D crowd moves)
            p.end_vehicle_step()
            z.end_vehicle_step()
            for u, v in zip(p.vehicle_episodes(), z.vehicle_episodes()):
                assert _same(u, v)
    finally:
        p.close()
        z.close()


# ---- G3 ---------------------------------------------------------------------------------------------------------------------------------

def test_vehicle_episodes_change_nothing_else():
    out = []
    for on in (False, True):
        b = _build(episodes=on)
        try:
            b.set_vehicle_observation(4, 8.0)
            b.set_episodes([-1 if n == 0 else 0 for n in VC.SIZES], goal_radius=3.0, ped_radius=0.9, veh_radius=1.0, max_steps=4)
            b.set_row_episodes(True, goal_radius=3.0, ped_radius=0.9, veh_radius=1.0, max_steps=4)
            got = []
            for _ in range(3):
                b.run(3)
                if on:
                    b.end_vehicle_step()
                b.end_step()
                b.end_row_step()
                if on:
                    b.end_vehicle_step()
                got.append((b.state_arrays(), b.vehicle_observations(), b.episodes(), b.row_episodes(), [w for w, _ in b.waypoints()],
                            [np.concatenate([np.ravel(c) for c, _ in veh] + [np.ravel(r) for _, r in veh] + [np.zeros(0)])
                             for veh in b.dynamic_obstacles()],
                            [np.concatenate([np.ravel(x) for x in drv]) for drv in b.vehicle_driving()]))
            out.append(got)
        finally:
            b.close()
    for u, v in zip(*out):
        for part_u, part_v in zip(u, v):
            assert len(part_u) == len(part_v) and all(_same(x, y) for x, y in zip(part_u, part_v))


# ---- G4 ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["host", "device", "end_step", "end_vehicle_step"])
def test_a_scene_restart_starts_the_vehicle_episodes_of_the_restarted_scenes_over(path):
    import torch
    restarted = np.zeros(VC.B, bool)
    restarted[[1, 3, 5, 8, 12]] = True
    b = _build()
    try:
        if path == "end_step":
            b.set_episodes([-1 if n == 0 else 0 for n in VC.SIZES], max_steps=[1 if r else 0 for r in restarted])
        b.snapshot()
        ages, prevs = [None] * b.B, [None] * b.B
        b.run(1)
        _evaluate(b, ALL, ages, prevs)
        if path == "end_vehicle_step":
            b.run(1)
            _evaluate(b, ALL, ages, prevs, auto_restart=True)
            restarted = b.vehicle_episodes()[2].copy()
            assert restarted.any() and not restarted.all()
        else:
            _evaluate(b, ALL, ages, prevs)
            if path == "host":
                b.restart(restarted)
            elif path == "device":
                b.restart_device(torch.as_tensor(restarted, device="cuda"))
            else:
                b.end_step(auto_restart=True)
                assert np.array_equal(b.episodes()[1], restarted)
        for k in ALL:                                                   # what the twin holds for a restarted scene: age 0, prev NaN
            if restarted[k]:
                ages[k], prevs[k] = None, None
        rec = _evaluate(b, ALL, ages, prevs)                            # ... and the next evaluation agrees, scene by scene
        for k in ALL:
            ag = VC.agents()[k]
            assert (rec[k][ag, 2] == (1.0 if restarted[k] else 3.0)).all(), f"scene {k}"
    finally:
        b.close()


def _after_restart(how):
    import torch
    b = _build()
    try:
        b.snapshot()
        b.run(2)
        if how == "auto":
            b.end_vehicle_step(auto_restart=True)
        else:
            b.end_vehicle_step()
            sd = b.vehicle_scene_done_tensor()
            assert 0 < int(sd.sum()) < b.B
            b.restart_device(sd if how == "own" else sd.clone().bool())
        b.run(1)
        b.end_vehicle_step()
        out = (b.state_arrays(), [w for w, _ in b.waypoints()], b.vehicle_episodes(),
               [np.concatenate([np.ravel(x) for x in drv]) for drv in b.vehicle_driving()],
               [np.concatenate([np.ravel(c) for c, _ in veh] + [np.ravel(r) for _, r in veh] + [np.zeros(0)]) for veh in b.dynamic_obstacles()])
        torch.cuda.synchronize()
        return out
    finally:
        b.close()


def test_the_auto_restart_the_own_mask_and_a_torch_mask_give_the_same():
    a, own, t = (_after_restart(how) for how in ("auto", "own", "torch"))
    for other in (own, t):
        for u, v in zip(a, other):
            assert len(u) == len(v) and all(_same(x, y) for x, y in zip(u, v))


# ---- G5 ---------------------------------------------------------------------------------------------------------------------------------

def _read(b, autopilot):
    """Per scene the dict scenarios.respawn_vehicles_scene takes, and everything else readable beside it."""
    cur = [c for c, _ in b.vehicle_autopilot()] if autopilot else [None] * b.B
    out = []
    for k, ((loc, vel), (wp, draws), veh, drv) in enumerate(zip(b.state(), b.waypoints(), b.dynamic_obstacles(), b.vehicle_driving())):
        d = {"centers": np.array([c for c, _ in veh]).reshape(-1, 2), "vel": drv[3], "headings": drv[2], "rings": [r for _, r in veh],
             "loc": loc, "pvel": vel, "wp": wp, "draws": draws, "kind": drv[0], "cmd": drv[1]}
        if autopilot:
            d["cursor"] = cur[k]
        out.append(d)
    return out


def _masks(which):
    none = [np.zeros(m, bool) for m in VC.VEHICLES]
    one = [m.copy() for m in none]
    one[4][5] = True
    scene = [m.copy() for m in none]
    scene[3][:] = True
    third = [np.arange(m) % 3 == 0 for m in VC.VEHICLES]
    return {"none": none, "one": one, "scene": scene, "third": third}[which]


@pytest.mark.parametrize("autopilot", [False, True])
@pytest.mark.parametrize("which", ["none", "one", "scene", "third"])
def test_respawn_copies_the_chosen_vehicles_only(which, autopilot):
    import torch
    chosen = _masks(which)
    b = _build(tracks=False, autopilot=autopilot)
    try:
        b.snapshot()
        snap = _read(b, autopilot)
        ages, prevs = [None] * b.B, [None] * b.B
        b.run(3)
        _evaluate(b, ALL, ages, prevs)
        _evaluate(b, ALL, ages, prevs)
        before = _read(b, autopilot)
        if autopilot:
            assert any((s["cursor"] != n["cursor"]).any() for s, n in zip(snap, before))      # the cursors have moved since the snapshot
        b.respawn_vehicles_device(torch.as_tensor(np.concatenate(chosen), device="cuda"))
        after = _read(b, autopilot)
        torch.cuda.synchronize()
        for k in ALL:
            want = scenarios.respawn_vehicles_scene(chosen[k], snap[k], dict(before[k], age=ages[k], prev=prevs[k]))
            for name, u in after[k].items():
                if name == "cmd" and autopilot:
                    continue                                            # (the controller's next launch writes the autopiloted commands)
                if name == "rings":
                    assert len(u) == len(want[name]) and all(_same(p, q) for p, q in zip(u, want[name])), f"{which}: scene {k}: rings"
                else:
                    assert _same(u, want[name]), f"{which}: scene {k}: {name}"
            ages[k], prevs[k] = want["age"], want["prev"]
        if which != "none":
            assert any((a["centers"] != c["centers"]).any() for a, c in zip(after, before))
        rec = _evaluate(b, ALL, ages, prevs)                            # the respawned vehicles' episodes started over, only theirs
        for k in ALL:
            ag = VC.agents()[k]
            assert (rec[k][ag & chosen[k], 2] == 1.0).all() and (rec[k][ag & ~chosen[k], 2] == 3.0).all()
        b.run(2)                                                        # ... and the scenes go on
    finally:
        b.close()


def test_vehicle_done_a_torch_mask_and_the_auto_respawn_give_the_same():
    import torch
    out = []
    for how in ("none", "torch", "auto"):
        b = _build(tracks=False)
        try:
            b.snapshot()
            b.run(3)
            if how == "auto":
                b.end_vehicle_step(auto_respawn=True)
            else:
                b.end_vehicle_step()
                done = b.vehicle_done_tensor()
                assert int(done.sum()) > 3
                b.respawn_vehicles_device(None if how == "none" else done.clone().bool())
            rec, done, _ = b.vehicle_episodes()
            assert done.any() and rec[done, 0].all()                    # the record keeps the terminal values
            b.end_vehicle_step()
            out.append((_read(b, False), b.vehicle_episodes()))
            torch.cuda.synchronize()
        finally:
            b.close()
    for other in out[1:]:
        for u, v in zip(out[0][0], other[0]):
            assert all(_same(np.concatenate([np.ravel(r) for r in u[n]] + [np.zeros(0)]) if n == "rings" else u[n],
                             np.concatenate([np.ravel(r) for r in v[n]] + [np.zeros(0)]) if n == "rings" else v[n]) for n in u)
        assert all(_same(u, v) for u, v in zip(out[0][1], other[1]))


# ---- G6 ---------------------------------------------------------------------------------------------------------------------------------

def test_views_alias_the_buffers():
    import torch
    b = _build()
    try:
        M = int(b._dyn[0][-1])
        rec_t, done_t, sd_t = b.vehicle_episode_tensor(), b.vehicle_done_tensor(), b.vehicle_scene_done_tensor()
        assert tuple(rec_t.shape) == (M, EPISODE_WIDTH) and rec_t.dtype == torch.float32
        assert tuple(done_t.shape) == (M,) and done_t.dtype == torch.uint8 and tuple(sd_t.shape) == (b.B,) and sd_t.dtype == torch.uint8
        assert b.device_ptr(PTR_VEHICLE_EPISODES) == (rec_t.data_ptr(), 32 * M) and b.device_ptr(PTR_VEHICLE_DONE) == (done_t.data_ptr(), M)
        assert b.device_ptr(PTR_VEHICLE_SCENE_DONE) == (sd_t.data_ptr(), b.B)
        b.run(1)
        b.end_vehicle_step()
        rec, done, sd = b.vehicle_episodes()
        assert _same(rec_t.cpu().numpy(), rec) and np.array_equal(done_t.cpu().numpy().astype(bool), done) and done.any()
        assert np.array_equal(sd_t.cpu().numpy().astype(bool), sd) and sd.any()
        b.set_vehicle_episodes(None)
        assert not b.has_vehicle_episodes
        with pytest.raises(SfmLibraryError, match="vehicle episodes are off"):
            b.vehicle_episode_tensor()
    finally:
        b.close()


def _everything(b):
    out = [b.state_arrays(), [w for w, _ in b.waypoints()], [np.concatenate([np.ravel(x) for x in drv]) for drv in b.vehicle_driving()]]
    if b.has_vehicle_episodes:
        out.append(b.vehicle_episodes())
    return out


def _unchanged(u, v):
    return len(u) == len(v) and all(len(p) == len(q) and all(_same(x, y) for x, y in zip(p, q)) for p, q in zip(u, v))


def _c_args(b, **change):
    """The nine arrays of sfm_batch_set_vehicle_episodes, every vehicle an agent, with one of them replaced."""
    M = int(b._dyn[0][-1])
    a = dict(agents=np.ones(M, np.uint8), gx=np.zeros(M, np.float32), gy=np.zeros(M, np.float32), ext=np.tile(np.float32(VC.EXTENT), (M, 1)),
             rg=np.ones(b.B, np.float32), rp=np.ones(b.B, np.float32), rv=np.ones(b.B, np.float32), rw=np.ones(b.B, np.float32),
             ms=np.zeros(b.B, np.int32))
    a.update(change)
    return a


def _c_set(b, **change):
    a = _c_args(b, **change)
    return b._lib.sfm_batch_set_vehicle_episodes(b._b, u8ptr(a["agents"]), fptr(a["gx"]), fptr(a["gy"]), fptr(np.ascontiguousarray(a["ext"])),
                                                 fptr(a["rg"]), fptr(a["rp"]), fptr(a["rv"]), fptr(a["rw"]), iptr(a["ms"]))


def test_refusals_change_nothing():
    fresh = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), [VC.DTS[k] for k in ALL])
    try:
        L = fresh._lib
        one, r, ms = np.ones(1, np.uint8), np.ones(VC.B, np.float32), np.zeros(VC.B, np.int32)
        call = lambda: L.sfm_batch_set_vehicle_episodes(fresh._b, u8ptr(one), fptr(r), fptr(r), fptr(r), fptr(r), fptr(r), fptr(r), fptr(r), iptr(ms))
        assert call() == SFM_ERR_STATE                                  # before upload
        fresh.upload(list(VC.scenes()))
        assert call() == SFM_ERR_STATE                                  # the vehicles are rings that stay: no device-side vehicles
        with pytest.raises(SfmLibraryError, match="device-side vehicles"):
            fresh.set_vehicle_episodes(True, goals=np.zeros(2), extents=np.ones(2))
    finally:
        fresh.close()
    b = _build()                                                        # tracks are set
    try:
        b.run(1)
        b.end_vehicle_step()
        held = _everything(b)
        M = int(b._dyn[0][-1])
        for bad in (-1.0, np.nan, np.inf, 2.0e6):                       # a bad radius, each of the four
            for name in ("rg", "rp", "rv", "rw"):
                r = np.ones(b.B, np.float32)
                r[3] = bad
                assert _c_set(b, **{name: r}) == SFM_ERR_INVALID
            with pytest.raises(ValueError):
                b.set_vehicle_episodes(True, goals=np.zeros(2), extents=np.ones(2), wall_radius=[bad if k == 3 else 1.0 for k in ALL])
        for bad in (0.0, -1.0, np.nan, np.inf, 2.0e6):                  # a bad extent of an agent
            e = np.tile(np.float32(VC.EXTENT), (M, 1))
            e[M - 1, 1] = bad
            assert _c_set(b, ext=e) == SFM_ERR_INVALID
        g = np.zeros(M, np.float32)
        g[2] = np.nan
        assert _c_set(b, gx=g) == SFM_ERR_INVALID
        neg = np.zeros(b.B, np.int32)
        neg[2] = -1
        assert _c_set(b, ms=neg) == SFM_ERR_INVALID
        assert b.has_vehicle_episodes and _unchanged(held, _everything(b))
        L = b._lib
        assert L.sfm_batch_end_vehicle_step(b._b, 3) == SFM_ERR_INVALID                                  # both flags
        assert L.sfm_batch_end_vehicle_step(b._b, 4) == SFM_ERR_INVALID
        assert L.sfm_batch_end_vehicle_step(b._b, 1) == SFM_ERR_STATE and L.sfm_batch_end_vehicle_step(b._b, 2) == SFM_ERR_STATE   # no snapshot
        assert L.sfm_batch_respawn_vehicles_device(b._b, None) == SFM_ERR_STATE
        with pytest.raises(SfmLibraryError, match="no snapshot"):
            b.respawn_vehicles_device()
        b.snapshot()
        assert L.sfm_batch_respawn_vehicles_device(b._b, None) == SFM_ERR_STATE                          # tracks are set
        with pytest.raises(SfmLibraryError, match="tracks are set"):
            b.respawn_vehicles_device()
        with pytest.raises(SfmLibraryError, match="tracks are set"):
            b.end_vehicle_step(auto_respawn=True)
        assert _unchanged(held, _everything(b))                         # nothing was launched: the ages did not move
        b.set_dynamic_boxes(VC.boxes())                                 # new vehicles drop the episodes
        assert not b.has_vehicle_episodes and L.sfm_batch_end_vehicle_step(b._b, 0) == SFM_ERR_STATE
    finally:
        b.close()
    b = _build(tracks=False)
    try:
        L = b._lib
        b.snapshot()
        held = _everything(b)[:3]
        b.set_vehicle_episodes(None)
        assert b.has_snapshot                                           # switching them off keeps the snapshot
        assert L.sfm_batch_respawn_vehicles_device(b._b, None) == SFM_ERR_INVALID                        # a NULL mask while they are off
        assert L.sfm_batch_end_vehicle_step(b._b, 0) == SFM_ERR_STATE
        assert L.sfm_batch_download_vehicle_episodes(b._b, None, None, None) == SFM_ERR_STATE
        for which in (PTR_VEHICLE_EPISODES, PTR_VEHICLE_DONE, PTR_VEHICLE_SCENE_DONE):                   # the new ids while the feature is off
            assert not L.sfm_batch_device_ptr(b._b, which, None)
            with pytest.raises(SfmLibraryError, match="which must be"):
                b.device_ptr(which)
        assert _unchanged(held, _everything(b))
        b.set_vehicle_episodes(**VC.episode_args())                     # setting them keeps the snapshot too
        assert b.has_snapshot and L.sfm_batch_respawn_vehicles_device(b._b, None) == 0
        b.upload(list(VC.scenes()))                                     # upload drops them
        assert not b.has_vehicle_episodes and L.sfm_batch_end_vehicle_step(b._b, 0) == SFM_ERR_STATE
    finally:
        b.close()


# ---- G7 ---------------------------------------------------------------------------------------------------------------------------------

def _reading(b):
    out = []
    for _ in range(2):
        b.run(1)
        b.end_vehicle_step()
        out.append(b.vehicle_episodes())
    return out


def test_a_used_batch_with_the_feature_dropped_and_set_again_reads_what_a_fresh_batch_reads():
    fresh = _build()
    try:
        want = _reading(fresh)
    finally:
        fresh.close()
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), [VC.DTS[k] for k in ALL])
    try:
        other = ALL[1:] + ALL[:1]                                       # another crowd first: the scenes in another order
        b.upload([VC.scenes()[k] for k in other])
        b.set_dynamic_boxes(VC.boxes(other))
        b.set_vehicle_driving(*_driving(other, False))
        b.set_vehicle_episodes(**VC.episode_args(other))
        b.snapshot()
        b.run(2)
        b.end_vehicle_step(auto_respawn=True)
        b.end_vehicle_step(auto_restart=True)
        b.upload(list(VC.scenes()))                                     # ... then this one
        assert not b.has_vehicle_episodes
        b.set_dynamic_boxes(VC.boxes())
        b.set_vehicle_tracks(VC.tracks())
        b.set_vehicle_driving(*_driving(ALL, True))
        b.set_vehicle_episodes(True, goals=np.zeros(2), extents=np.ones(2), goal_radius=9.0, max_steps=1)
        b.end_vehicle_step()
        b.set_vehicle_episodes(None)                                    # dropped ...
        b.set_vehicle_episodes(**VC.episode_args())                     # ... and set again
        got = _reading(b)
        for g, w in zip(got, want):
            assert all(_same(u, v) for u, v in zip(g, w))
    finally:
        b.close()
