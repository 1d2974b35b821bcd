"""GPU tests of per-pedestrian observations on a batch (sfm_batch_set_observation, sfm_batch_observe, sfm_batch_download_observations,
sfm_batch_observation_ptr; SfmBatch.set_observation / observe / observations / observation_tensor): bitwise against the host twin
``observe.observe_scene`` in frame 0, ties, the heading frame within a derived bound, independence of the rest of the batch, that
observing changes nothing, ghosts and traffic, restarts, the device view, and every refusal."""
import ctypes as C
import importlib.util
import os
from functools import lru_cache

import numpy as np
import pytest

import test_batch_gpu as G
import test_batch_modes_gpu as M
import test_batch_tracks_gpu as T
import test_batch_vehicles_gpu as V
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd._lib import SfmLibraryError
from carla_social_force_model_amd.batch import OBS_HEADER, SfmBatch
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.observe import candidate_counts, heading, observe_scene, rotate_record

pytestmark = pytest.mark.gpu

SFM_ERR_INVALID, SFM_ERR_STATE = -1, -3
SIZES = (0, 1, 2, 3, 17, 64, 65, 128, 129, 256, 257, 300, 1024, 40, 90)      # the last two carry 3 vehicles each
RANGES = (2.0, 3.0, 5.0)
KS = (1, 4, 8, 16)
U = 2.0 ** -24


def _ranges(B):
    return [RANGES[b % 3] for b in range(B)]


@lru_cache(maxsize=None)
def _scenes(z3=False):
    """The mixed batch.  The 3-D form has the planar form's x, y, vx, vy, with a z and a vz of its own per row."""
    scenes = [G._scene(n, 4000 + q, dynamic=3 if q >= 13 else 0) for q, n in enumerate(SIZES)]
    if z3:
        rng = np.random.default_rng(5)
        for sc in scenes:
            n = len(sc["loc"])
            sc["loc"] = np.column_stack([sc["loc"][:, :2], rng.uniform(0.0, 1.5, n)])
            sc["vel"] = np.column_stack([sc["vel"][:, :2], rng.uniform(-0.2, 0.2, n)])
    return scenes


@lru_cache(maxsize=None)
def _twin(k):
    return [observe_scene(sc, k, R) for sc, R in zip(_scenes(), _ranges(len(SIZES)))]


def _batch(scenes, planar=None, device_vehicles=False):
    b = SfmBatch(default_sfm_config(), 0.05, B=len(scenes))
    b.upload(scenes, planar=planar, device_vehicles=device_vehicles)
    return b


def _observed(scenes, k, ranges, frame=0, planar=None):
    b = _batch(scenes, planar)
    try:
        b.set_observation(k, ranges, frame)
        return b.observations()
    finally:
        b.close()


@lru_cache(maxsize=None)
def _device(k, z3, frame=0):
    return _observed(_scenes(z3), k, _ranges(len(SIZES)), frame)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.array_equal(got, want), f"{what}: rows {np.flatnonzero((got != want).any(axis=1))[:5]}"


# ---- 1. bitwise against the twin, frame 0 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_the_batch_holds_every_class_of_row(k):
    """From the twin alone: rows with no neighbour, with fewer than k (k > 1: with k = 1 there is no count between 0 and k),
    with exactly k candidates and with more; for each geometry kind a row that sees a point and one that does not."""
    scenes, R = _scenes(), _ranges(len(SIZES))
    cnt = np.concatenate([candidate_counts(sc, r) for sc, r in zip(scenes, R)])
    rec = np.concatenate(_twin(k))
    assert np.array_equal(rec[:, 6], np.minimum(cnt, k))
    assert (cnt == 0).any() and (cnt == k).any() and (cnt > k).any()
    assert k == 1 or ((cnt > 0) & (cnt < k)).any()
    flags = rec[:, 7].astype(np.int64)
    for bit in (1, 2, 4):
        assert ((flags & bit) != 0).any() and ((flags & bit) == 0).any(), bit


@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
@pytest.mark.parametrize("k", KS)
def test_frame0_is_bitwise_the_twin(k, z3):
    got, want = _device(k, z3), _twin(k)
    assert len(got) == len(SIZES)
    for s, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"scene {s} (N = {SIZES[s]})")


# ---- 2. ties and degenerate rows ------------------------------------------------------------------------------------------------

def _lattice():
    xy = np.array([[c, r] for r in range(5) for c in range(5)], dtype=np.float64)
    sc = G._scene(25, 77, geo=False)
    sc["loc"] = np.column_stack([xy, np.zeros(25)])
    return sc


def test_ties_and_a_coincident_pair():
    lat = _lattice()
    pair = G._scene(17, 4100)
    pair["loc"] = np.array(pair["loc"])
    pair["loc"][6] = pair["loc"][5]
    for k in (4, 8):
        got = _observed([lat, pair], k, [1.5, 3.0])
        _same(got[0], observe_scene(lat, k, 1.5), f"lattice, k = {k}")
        _same(got[1], observe_scene(pair, k, 3.0), f"coincident pair, k = {k}")
        d = got[0][12, OBS_HEADER:].reshape(k, 4)[:, :2]
        want = [(0, -1), (-1, 0), (1, 0), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)][:k]      # rows 7, 11, 13, 17, then 6, 8, 16, 18
        assert np.array_equal(d, np.float32(want)) and got[0][12, 6] == k
        assert not got[1][5, OBS_HEADER:OBS_HEADER + 2].any() and got[1][5, 6] >= 1


# ---- 3. frame 1 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 16])
def test_heading_frame(k):
    """m, flags, target speed and live are those of frame 0; every rotated vector (a, b) lies within 8 * 2^-24 * (|a| + |b|) per
    component of the float64 rotation by the twin's heading.  The bound is derived: 3 * 2^-24 relative on each of h_x, h_y (one fma
    and its product, a correctly rounded sqrt, a correctly rounded divide), one rounded product and the final rounding of the fma
    give 5 * 2^-24 * (|a| + |b|); the rest is headroom for an rsq-based form.  A slot that held another neighbour, or the same
    neighbours in another order, would miss it by metres."""
    zero = G._scene(17, 4200)
    zero["vel"] = np.array(zero["vel"])
    zero["vel"][3] = 0.0                                                # heading from the goal
    zero["vel"][4] = 0.0
    zero["waypoint"] = np.array(zero["waypoint"])
    zero["waypoint"][4] = zero["loc"][4]                                # ... and (1, 0) without one
    f0 = _device(k, False) + _observed([zero], k, [3.0])
    f1 = _device(k, False, 1) + _observed([zero], k, [3.0], frame=1)
    assert np.array_equal(f0[-1], observe_scene(zero, k, 3.0))
    worst = 0.0
    for s, (a, b) in enumerate(zip(f0, f1)):
        assert np.array_equal(a[:, 4:8], b[:, 4:8]), f"scene {s}: target speed, live, m, flags"
        want = rotate_record(a, heading(a))
        a64 = a.astype(np.float64)
        for c in [0, 2] + list(range(8, a.shape[1], 2)):
            bound = 8 * U * (np.abs(a64[:, c]) + np.abs(a64[:, c + 1]))
            err = np.abs(b[:, c:c + 2].astype(np.float64) - want[:, c:c + 2])
            worst = max(worst, float((err / np.maximum(bound, 1e-300)[:, None]).max(initial=0.0)))
            assert (err <= bound[:, None]).all(), f"scene {s}, floats {c}-{c + 1}: rows {np.flatnonzero((err > bound[:, None]).any(axis=1))[:5]}"
    print(f"heading frame, k = {k}: worst error / bound = {worst:.3f}")
    assert np.array_equal(f1[-1][4], f0[-1][4])                          # heading (1, 0): the record is that of frame 0
    sp = np.linalg.norm(f0[12][:, 2:4].astype(np.float64), axis=1)
    assert np.all(np.abs(f1[12][:, 2] - sp) <= 8 * U * 2 * sp) and np.all(np.abs(f1[12][:, 3]) <= 8 * U * 2 * sp)


# ---- 4. independence ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("z3", [False, True], ids=["planar", "3d"])
def test_a_scene_does_not_depend_on_the_rest_of_the_batch(z3):
    scenes, R = _scenes(z3), _ranges(len(SIZES))
    k = 8
    mixed = _device(k, z3)
    for s in (14, 9):                                                   # 90 rows with vehicles; 256 rows
        alone = _observed([scenes[s]], k, [R[s]], planar=not z3)
        moved = _observed([scenes[4], scenes[s], scenes[0], scenes[3]], k, [5.0, R[s], 2.0, 2.0], planar=not z3)
        assert np.array_equal(_bits(alone[0]), _bits(mixed[s])), f"scene {s} alone"
        assert np.array_equal(_bits(moved[1]), _bits(mixed[s])), f"scene {s} at position 1 of another batch"


def test_a_3d_batch_gives_the_planar_record():
    for k in (1, 16):
        for s, (a, b) in enumerate(zip(_device(k, False), _device(k, True))):
            assert np.array_equal(_bits(a), _bits(b)), f"k = {k}, scene {s}"


# ---- 5. observing changes nothing -----------------------------------------------------------------------------------------------

def _modes_batch():
    made = [M._scene(n, 4300 + q, 2 if n else 1) for q, n in enumerate((64, 0, 130, 17))]
    scenes, plans = [m[0] for m in made], [m[1] for m in made]
    return M._batch(scenes, plans, [M._config(q) for q in range(4)], [0.05, 0.04, 0.03, 0.05])


def _all(b):
    rows, clocks = M._everything(b)
    return rows, clocks, [[np.concatenate([c.reshape(-1), r.reshape(-1)]) for c, r in veh] for veh in b.dynamic_obstacles()]


def _assert_all(x, y, what):
    M._assert_same(x[:2], y[:2], what)
    for k, (u, v) in enumerate(zip(x[2], y[2])):
        assert len(u) == len(v) and all(np.array_equal(p, q) for p, q in zip(u, v)), f"{what}: vehicles of scene {k}"


def test_observing_changes_nothing():
    a, b = _modes_batch(), _modes_batch()
    try:
        a.set_observation(8, 3.0, 1)
        a.run(3)
        before = _all(a)
        a.observe()
        first = a.observations()
        _assert_all(_all(a), before, "state, waypoints, modes, clocks, vehicles around observe()")
        a.run(5)
        a.observe()
        a.run(5)
        b.run(13)
        _assert_all(_all(a), _all(b), "run(3), observe, run(5), observe, run(5) against run(13)")
        assert any((x != y).any() for x, y in zip(first, a.observations()) if len(x))
    finally:
        a.close()
        b.close()


# ---- 6. ghosts and traffic ------------------------------------------------------------------------------------------------------

def test_ghosts_are_zero_and_nobodys_neighbour():
    """Modes, despawn on arrival and a spawn schedule, run until a row has despawned while another is still unborn: their records
    are zero, no live row lists them (the twin, fed with the state, says who is listed), the rest equals the twin.  The target
    speed a record holds is the one the last tick applied -- the mode target before that tick -- so the modes are read one tick
    before the end (a row born in the last tick: the target of its plan)."""
    sizes = (64, 17, 130)
    made = [M._scene(n, 4400 + q, 2) for q, n in enumerate(sizes)]
    scenes, plans = [m[0] for m in made], [m[1] for m in made]
    scheds = [scenarios.make_spawn_plan(sc, 9 + q, horizon=6.0) for q, sc in enumerate(scenes)]
    for sd in scheds:
        sd["spawn_time"][-1] = np.inf                                   # never born
        sd["chain"][-1] = 0
    b = M._batch(scenes, plans, [M._config(q) for q in range(3)], [0.05, 0.04, 0.05])
    try:
        b.set_spawns(scheds)
        b.set_observation(8, 4.0)
        found = False
        for _ in range(100):
            b.run(9)
            prev = [t.copy() for _, t, _ in b.modes()]
            born_prev = [bn.copy() for bn, _ in b.spawns()]
            b.run(1)
            modes = [m for m, _, _ in b.modes()]
            if all((m == M.GONE).any() for m in modes) and all((m == 254).any() for m in modes):
                found = True
                break
        assert found, "no tick with a despawned and an unborn row in every scene"
        obs = b.observations()
        for s, ((loc, vel), (wp, _), (born, _)) in enumerate(zip(b.state(), b.waypoints(), b.spawns())):
            ghost = (modes[s] == M.GONE) | (modes[s] == 254)
            assert ghost.any() and not ghost.all()
            assert not obs[s][ghost].any(), f"scene {s}: a ghost's record"
            ts = np.where(born & ~born_prev[s], np.float32(plans[s]["target_speed"]), prev[s])
            want = observe_scene(scenes[s], 8, 4.0, state=(loc, vel), vehicles=b.dynamic_obstacles()[s], waypoints=wp, target_speed=ts)
            _same(obs[s], want, f"scene {s}")
            assert np.array_equal(obs[s][:, 5] == 0, ghost)
    finally:
        b.close()


def test_vehicles_as_the_next_tick_reads_them():
    """Device-side vehicles after run(7): the records equal the twin fed with dynamic_obstacles() and the boxes' velocities.
    Tracked vehicles outside their keyframes are absent: bit 4 is clear for everyone."""
    scenes = [V._scene(n, 4500 + q, m, slow=False) for q, (n, m) in enumerate(((64, 3), (30, 2), (0, 1), (130, 5)))]
    b = V._batch(scenes, [V._config(q, V.ALL) for q in range(4)], [0.05, 0.04, 0.05, 0.03])
    try:
        b.set_observation(4, 6.0)
        b.run(7)
        obs, veh = b.observations(), b.dynamic_obstacles()
        for s, (loc, vel) in enumerate(b.state()):
            _same(obs[s], observe_scene(scenes[s], 4, 6.0, state=(loc, vel), vehicles=veh[s]), f"scene {s} after run(7)")
        assert any((o[:, 7].astype(np.int64) & 4).any() for o in obs)
        # tracks: scene 0's vehicles leave after 3, 5 and 4 keyframes; every other scene's run free
        rng = np.random.default_rng(3)
        tracks = [[T._track(rng, 3, 0, T._mid(scenes[0])), T._track(rng, 5, 0, T._mid(scenes[0])), T._track(rng, 4, 0, T._mid(scenes[0]))],
                  None, None, None]
        b.set_vehicle_tracks(tracks)
        b.set_observation(4, 1.0e6)                                     # everyone sees whatever is there
        for tau, gone in ((0, False), (2, False), (4, False), (6, True)):
            while b.vehicle_tracks()[0] < tau:
                b.run(1)
            obs, veh = b.observations(), b.dynamic_obstacles()
            twin_sc = dict(scenes[0])
            scenarios.place_tracked(twin_sc, tracks[0], tau)
            assert twin_sc["dynamic_present"].any() != gone
            loc, vel = b.state()[0]
            want = observe_scene(scenes[0], 4, 1.0e6, state=(loc, vel), vehicles=veh[0], vehicle_vel=twin_sc["dynamic_vel"])
            _same(obs[0], want, f"tracked scene at tau = {tau}")
            bit = (obs[0][:, 7].astype(np.int64) & 4) != 0
            assert bit.all() != gone and bit.any() != gone
            assert not gone or not obs[0][:, 8:12].any()
            assert ((obs[3][:, 7].astype(np.int64) & 4) != 0).all()      # the free vehicles of another scene are still seen
    finally:
        b.close()


# ---- 7. restart -----------------------------------------------------------------------------------------------------------------

def test_restarted_scenes_read_what_they_read_at_the_snapshot():
    scenes = [G._scene(n, 4600 + q) for q, n in enumerate((30, 65, 0, 130, 17))]
    b = _batch(scenes)
    try:
        b.set_observation(8, [2.0, 3.0, 5.0, 3.0, 5.0])
        b.run(3)
        b.snapshot()
        at_snapshot = b.observations()
        b.run(20)
        b.restart([1, 3])
        assert b.has_snapshot
        obs = b.observations()
        for s, (loc, vel) in enumerate(b.state()):
            if s in (1, 3):
                assert np.array_equal(_bits(obs[s]), _bits(at_snapshot[s])), f"restarted scene {s}"
            else:
                _same(obs[s], observe_scene(scenes[s], 8, (2.0, 3.0, 5.0, 3.0, 5.0)[s], state=(loc, vel)), f"scene {s} went on")
                assert not len(obs[s]) or (obs[s] != at_snapshot[s]).any()
    finally:
        b.close()


# ---- 8. device view -------------------------------------------------------------------------------------------------------------

def test_device_view():
    import torch
    scenes = [G._scene(n, 4700 + q) for q, n in enumerate((17, 0, 65))]
    b = _batch(scenes)
    try:
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        b.set_observation(4, 3.0)
        nbytes = C.c_int64(0)
        ptr = b._lib.sfm_batch_observation_ptr(b._b, C.byref(nbytes))
        t = b.observation_tensor()
        assert t.shape == (82, 32) and t.dtype == torch.float32 and t.data_ptr() == ptr and nbytes.value == 82 * 32 * 4
        assert not t.any().item()                                       # zero-filled before the first observe
        b.run(2)
        b.observe()
        seen = t.cpu().numpy()                                          # (torch's stream: ordered behind the launch)
        assert np.array_equal(seen, np.concatenate(b.observations()))
        assert np.array_equal(seen, np.concatenate([observe_scene(sc, 4, 3.0, state=st) for sc, st in zip(scenes, b.state())]))
        b.set_observation(16, 3.0)                                      # a new buffer: the view is taken again
        assert b.observation_tensor().shape == (82, 80)
    finally:
        b.close()
    e = _batch([G._scene(0, 1)])                                        # without rows: no buffer, an empty view
    try:
        e.set_observation(4, 3.0)
        e.observe()
        assert e._lib.sfm_batch_observation_ptr(e._b, None) is None
        assert e.observation_tensor().shape == (0, 32) and e.observations()[0].shape == (0, 32)
    finally:
        e.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_batch_usable():
    scenes = [G._scene(n, 4800 + q) for q, n in enumerate((17, 65))]
    L = _lib.load()
    err = lambda x: L.sfm_batch_last_error(x._b).decode()
    r = np.float32([3.0, 5.0])
    b = SfmBatch(default_sfm_config(), 0.05, B=2)
    try:
        assert L.sfm_batch_set_observation(b._b, 4, _lib.fptr(r), 0) == SFM_ERR_STATE and "sfm_batch_upload_state" in err(b)
        with pytest.raises(SfmLibraryError, match="upload"):
            b.set_observation(4, 3.0)
        b.upload(scenes)

        def off(what):
            assert L.sfm_batch_observe(b._b) == SFM_ERR_STATE and "observations are off" in err(b), what
            out = np.zeros(82 * 32, np.float32)
            assert L.sfm_batch_download_observations(b._b, _lib.fptr(out)) == SFM_ERR_STATE and "observations are off" in err(b), what
            nbytes = C.c_int64(7)
            assert L.sfm_batch_observation_ptr(b._b, C.byref(nbytes)) is None and nbytes.value == 0 and "observations are off" in err(b), what
            for call in (b.observe, b.observations, b.observation_tensor):
                with pytest.raises(SfmLibraryError, match="observations are off"):
                    call()

        def usable(what):
            got = b.observations()
            for s, (loc, vel) in enumerate(b.state()):
                _same(got[s], observe_scene(scenes[s], 4, float(r[s]), state=(loc, vel)), f"{what}: scene {s}")
            b.run(2)

        off("before set_observation")
        for k in (0, 17, -1):
            assert L.sfm_batch_set_observation(b._b, k, _lib.fptr(r), 0) == SFM_ERR_INVALID and "k must be" in err(b)
        for frame in (2, -1):
            assert L.sfm_batch_set_observation(b._b, 4, _lib.fptr(r), frame) == SFM_ERR_INVALID and "frame must be" in err(b)
        for bad in (np.nan, 0.0, -1.0, np.inf, 2.0e6):
            assert L.sfm_batch_set_observation(b._b, 4, _lib.fptr(np.float32([3.0, bad])), 0) == SFM_ERR_INVALID
            assert "scene 1: sense_range" in err(b), bad
            with pytest.raises(ValueError, match="sense_range"):
                b.set_observation(4, [3.0, bad])
        off("after refused calls on a batch without observations")
        b.run(2)
        b.set_observation(4, r)
        usable("first settings")
        for args in ((0, r, 0), (17, r, 0), (4, r, 2), (4, np.float32([np.nan, 1.0]), 0), (4, np.float32([1.0, 2.0e6]), 1)):
            assert L.sfm_batch_set_observation(b._b, args[0], _lib.fptr(args[1]), args[2]) == SFM_ERR_INVALID
            usable(f"after the refused {args[0], args[2]}")                # nothing changed: k = 4, frame 0, the ranges
        b.snapshot()
        b.set_observation(4, r)                                          # keeps the snapshot
        assert b.has_snapshot
        b.restart()
        b.set_observation(None)
        off("after set_observation(None)")
        b.run(1)
        b.set_observation(4, r)
        usable("set again after off")
        b.upload(scenes)                                                 # drops the settings
        off("after upload")
        b.set_observation(4, r)
        usable("set again after upload")
    finally:
        b.close()


# ---- the example ----------------------------------------------------------------------------------------------------------------

def test_rl_loop_example_runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("batch_rl_loop", os.path.join(root, "examples", "batch_rl_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    episodes, arrivals = ex.run(B=8, steps=12, repeat=2, max_age=5, quiet=True)
    assert episodes >= 8 and 0 <= arrivals <= episodes                  # everyone runs out of time at least once
