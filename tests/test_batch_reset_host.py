"""Host tests of the batch's restart noise (sfm_batch_set_restart_noise): the random words against a plain-Python restatement, the
properties of the NumPy twin (``reset.resample_scene``) on designed and random scenes, that the crowd the GPU test uses is not
vacuous, the packer's refusals, and the entry points.  No GPU needed."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import _reset_cases as RC
from carla_social_force_model_amd import _lib, batch, reset, scenarios
from carla_social_force_model_amd.observe import _d2, range2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF


def _mix32(a):
    a ^= a >> 16; a = (a * 0x7FEB352D) & M32; a ^= a >> 15; a = (a * 0x846CA68B) & M32; a ^= a >> 16
    return a


def _word(seed, i, e, t, c):
    inner = _mix32(0x5BD1E995 ^ ((8 * i + c) & M32))
    return _mix32(seed ^ _mix32((inner + 0x9E3779B9 * ((32 * e + t) & M32)) & M32))


def _keys(count):
    rng = np.random.default_rng(5)
    keys = [(int(rng.integers(0, 2**32)), int(rng.integers(0, 1024)), int(rng.integers(0, 2**32)), int(rng.integers(0, 32)),
             int(rng.integers(0, 5))) for _ in range(count)]
    return keys + [(0, 0, 0, 0, 0), (M32, 1023, M32, 31, 4), (1, 0, 2**27, 0, 0)]


def test_random_words_agree_with_plain_integers():
    a = np.random.default_rng(1).integers(0, 2**32, 300, dtype=np.uint64)
    assert [int(v) for v in reset.mix32(a)] == [_mix32(int(v)) for v in a]
    for key in _keys(300):
        h = int(reset.reset_word(*key))
        assert h == _word(*key), key
        assert float(reset.unit(h)) == (h >> 8) / 2.0**24 and 0.0 <= float(reset.unit(h)) < 1.0
    cols = np.array(_keys(300), dtype=np.uint64).T                     # ... and as arrays
    assert [int(v) for v in reset.reset_word(*cols)] == [_word(*(int(v) for v in key)) for key in cols.T]


def test_offsets_stay_inside_the_half_open_box():
    for ext in (np.float32(0.1), np.float32(1.0), np.float32(0.75), np.float32(1.0e6), np.float32(1.1754944e-38)):
        for h in (0, 255, 256, M32, M32 - 255, 0x80000000):
            o = reset.offset(h, ext)
            assert o.dtype == np.float32 and -ext <= o < ext, (ext, h, o)
    assert reset.offset(0, np.float32(0.5)) == np.float32(-0.5)
    o = reset.offset(M32, np.float32(0.0))                              # a zero extent: +0, whatever the word
    assert o == 0.0 and not np.signbit(o)
    assert [reset.delay_ticks(h, 6) for h in (0, M32)] == [0, 6] and reset.delay_ticks(M32, 0) == 0


def _scene(xy, waypoint=None, **geo):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(xy)
    loc = np.column_stack([xy, np.zeros(n)])
    wp = loc + 5.0 if waypoint is None else np.column_stack([np.asarray(waypoint, dtype=np.float64).reshape(n, 2), np.zeros(n)])
    return dict({"loc": loc, "vel": np.zeros((n, 3)), "waypoint": wp, "target_speed": np.full(n, 1.2)}, **geo)


def _all_points(sc, vehicles):
    kinds = [np.asarray(p, np.float32).reshape(-1, 2) for p in sc.get("borders") or []]
    kinds += [np.asarray(r, np.float32).reshape(-1, 2) for _, r in (sc.get("static_obstacles") or [])]
    kinds += [np.asarray(r, np.float32).reshape(-1, 2) for _, r in vehicles]
    return np.concatenate(kinds) if kinds else np.zeros((0, 2), np.float32)


def _check_properties(sc, seed, e, pos, goal, gap, pgap, tries, **kw):
    xy, wp, first, veh, fb, det = reset.resample_scene(sc, seed, e, pos, goal, gap, pgap, tries, detail=True, **kw)
    x0 = np.asarray(sc["loc"], np.float64)[:, :2].astype(np.float32)
    w0 = np.asarray(sc["waypoint"], np.float64)[:, :2].astype(np.float32)
    n = len(x0)
    pos = np.broadcast_to(np.asarray(pos, np.float32), (n, 2))
    rnd = det["round"]
    alive = (np.abs(x0) < 1e12).all(axis=1)
    still = rnd < 0                                                    # not movable, or a fallback: where it was, bit for bit
    assert np.array_equal(xy[still].view(np.uint32), x0[still].view(np.uint32))
    assert (rnd[~alive] == reset.NOT_MOVABLE).all() and (rnd[alive & (pos == 0).all(axis=1)] == reset.NOT_MOVABLE).all()
    assert fb == int((rnd == reset.FALLBACK).sum())
    d = xy.astype(np.float64) - x0
    assert (np.abs(d[alive]) <= pos[alive]).all()                      # inside the box (the add rounds: <=)
    if goal is not None:
        g = np.broadcast_to(np.asarray(goal, np.float32), (n, 2))
        assert (np.abs(wp.astype(np.float64) - w0)[alive] <= g[alive] * (1 + 2.0**-20) + 1e-6).all()
        assert np.array_equal(wp[~alive].view(np.uint32), w0[~alive].view(np.uint32))
    else:
        assert np.array_equal(wp.view(np.uint32), w0.view(np.uint32))
    block = np.flatnonzero(alive & (rnd != reset.FALLBACK))            # fixed and accepted rows: every pair keeps the gap
    bx, by = xy[block, 0], xy[block, 1]
    d2 = _d2(bx[None, :] - bx[:, None], by[None, :] - by[:, None])
    off = ~np.eye(len(block), dtype=bool)
    movable_pair = (rnd[block] >= 0)[:, None] | (rnd[block] >= 0)[None, :]     # (two fixed rows were never checked)
    assert (d2[off & movable_pair] >= range2(gap)).all()
    pts = _all_points(sc, veh)
    acc = np.flatnonzero(rnd >= 0)
    if len(pts) and len(acc):
        d2p = _d2(xy[acc, 0][:, None] - pts[None, :, 0], xy[acc, 1][:, None] - pts[None, :, 1])
        assert (d2p >= range2(pgap)).all()
    return xy, wp, first, veh, fb, det


def test_twin_properties_on_the_shared_crowd_and_on_random_scenes():
    for k in range(len(RC.SIZES)):
        sc = RC.scenes()[k]
        pos, goal = RC.boxes()
        for e in (0, 1, 2):
            _check_properties(sc, RC.SEEDS[k], e, pos[k], goal[k], RC.MIN_GAP, RC.POINT_GAP, RC.TRIES, tracks=RC.tracks()[k],
                              track_delay=np.array([RC.DELAY, 3]) if RC.tracks()[k] else None, tau=4)
    for seed in range(6):
        sc = vars(scenarios.make_scenario(40 + 7 * seed, 700 + seed, n_borders=2, n_static=1, n_dynamic=1, border_len=(5.0, 9.0)))
        _check_properties(sc, seed, seed, np.array([0.8, 1.3], np.float32), np.array([2.0, 0.0], np.float32), 0.5, 0.25, 1 + 3 * seed)


def test_zero_gaps_accept_everybody_in_round_0_with_the_jitter_formula():
    sc = RC.scenes()[3]
    n = RC.SIZES[3]
    pos = np.array([0.5, 0.25], np.float32)
    xy, wp, _, _, fb, det = reset.resample_scene(sc, 77, 3, pos, np.array([1.0, 2.0]), 0.0, 0.0, 5, detail=True)
    assert fb == 0 and (det["round"] == 0).all() and det["rejected"] == {"blocker": 0, "lower": 0, "point": 0}
    x0 = sc["loc"][:, :2].astype(np.float32)
    for i in range(n):
        for c in (0, 1):
            u = np.float32((_word(77, i, 3, 0, c) >> 8) / 2.0**24)
            o = np.float32(np.float64(np.float32(2.0) * u) * np.float64(pos[c]) - np.float64(pos[c]))     # exact in double: one rounding
            assert xy[i, c] == np.float32(x0[i, c] + o)
    w0 = sc["waypoint"][:, :2].astype(np.float32)
    u = np.float32((_word(77, 5, 3, 0, 3) >> 8) / 2.0**24)
    assert wp[5, 1] == np.float32(w0[5, 1] + np.float32(np.float64(np.float32(2.0) * u) * 2.0 - 2.0))


def test_the_restart_counter_and_the_seed_key_the_draws():
    sc = RC.scenes()[3]
    pos, goal = RC.boxes()
    run = lambda seed, e: reset.resample_scene(sc, seed, e, pos[3], goal[3], RC.MIN_GAP, RC.POINT_GAP, RC.TRIES)
    a, b, c, d = run(404, 0), run(404, 0), run(404, 1), run(405, 0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
    assert not np.array_equal(a[0], d[0])


def test_a_scene_does_not_depend_on_its_batch():
    """The twin takes one scene: the batch is not among its arguments.  What a batch could leak is the row's index -- it must be the
    index inside the scene: the scene's result is the same whatever stands in front of it."""
    sc = RC.scenes()[3]
    pos, goal = RC.boxes()
    a = reset.resample_scene(sc, 404, 2, pos[3], goal[3], RC.MIN_GAP, RC.POINT_GAP, RC.TRIES)
    shuffled = [RC.scenes()[k] for k in (5, 3, 0)]
    b = [reset.resample_scene(s, 404, 2, RC.boxes()[0][k], RC.boxes()[1][k], RC.MIN_GAP, RC.POINT_GAP, RC.TRIES) for s, k in zip(shuffled, (5, 3, 0))][1]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[4] == b[4]


def test_designed_fallbacks():
    sc = _scene([[0.0, 0.0], [0.5, 0.0]])
    xy, _, _, _, fb, det = reset.resample_scene(sc, 9, 0, np.array([0.1, 0.1]), None, 1.0, 0.0, 8, detail=True)
    assert list(det["round"]) == [0, reset.FALLBACK] and fb == 1
    assert xy[1, 0] == np.float32(0.5) and xy[1, 1] == 0.0 and xy[0, 0] != 0.0
    th = 2.0 * np.pi * np.arange(60) / 60
    ring = np.column_stack([0.5 * np.cos(th), 0.5 * np.sin(th)])
    for kind in ({"borders": [ring], "border_centers": np.zeros((1, 2)), "border_lengths": np.array([6.0])},
                 {"static_obstacles": [(np.zeros(2), ring)]}, {"dynamic_obstacles": [(np.zeros(2), ring)]}):
        lone = _scene([[0.0, 0.0]], **kind)
        xy, _, _, _, fb, det = reset.resample_scene(lone, 9, 0, np.array([0.2, 0.2]), None, 0.0, 1.5, 8, detail=True)
        assert fb == 1 and det["rejected"] == {"blocker": 0, "lower": 0, "point": 8} and not xy.any()
        assert reset.resample_scene(lone, 9, 0, np.array([0.2, 0.2]), None, 0.0, 0.0, 8)[4] == 0     # a gap of 0 never rejects


def test_traffic_timing_moves_the_first_tick_and_places_the_vehicle_again():
    k = 3
    sc, tr = RC.scenes()[k], RC.tracks()[k]
    seen = set()
    for e in range(12):
        _, _, first, veh, _ = RC.twin(k, e, shift=3, tau=5)
        add = int(first[0]) - (tr[0]["first_tick"] + 3)
        assert add == reset.delay_ticks(_word(RC.SEEDS[k], 0, e, 0, 4), RC.DELAY) and 0 <= add <= RC.DELAY and first[1] == 0
        seen.add(add)
        want = scenarios.place_tracked(dict(sc), [dict(tr[0], first_tick=int(first[0])), None], 5)["dynamic_obstacles"][0]
        assert np.array_equal(veh[0][0], want[0]) and np.array_equal(veh[0][1], want[1])
        assert veh[1] is sc["dynamic_obstacles"][1]                    # the free-running vehicle: as it was fed in
    assert len(seen) > 2


def test_the_gpu_fixture_is_not_vacuous():
    movable = fallbacks = 0
    rejected = {"blocker": 0, "lower": 0, "point": 0}
    late = 0
    for k in range(len(RC.SIZES)):
        for e in (0, 1, 2):
            *_, fb, det = RC.twin(k, e, shift=3, tau=5, detail=True)
            movable += int((det["round"] != reset.NOT_MOVABLE).sum())
            fallbacks += fb
            late += int((det["round"] >= 2).sum())
            for key in rejected:
                rejected[key] += det["rejected"][key]
            if k == RC.ZERO_BOXES:
                assert (det["round"] == reset.NOT_MOVABLE).all()
            if k == RC.GHOSTS:
                assert (det["round"][[7, 200]] == reset.NOT_MOVABLE).all()
            if k == RC.DESIGNED:
                assert det["round"][0] == reset.NOT_MOVABLE and det["round"][1] == reset.FALLBACK
    print("movable", movable, "fallbacks", fallbacks, "placed in a round >= 2", late, rejected)
    assert all(v > 0 for v in rejected.values()) and late > 0 and fallbacks > 0
    assert 10 * fallbacks <= movable


def test_packer_refusals():
    so = np.array([0, 2, 5], dtype=np.int32)
    ok = dict(seeds=[1, 2], pos_box=np.array([0.5, 0.5]), scene_off=so)
    sd, phx, phy, ghx, ghy, g1, g2, tries, delay = batch.pack_restart_noise(**ok, goal_box=[np.zeros((2, 2)), np.array([1.0, 2.0])], min_gap=0.6,
                                                                              point_gap=[0.1, 0.2], tries=4, track_delay=[0, 5, 2], vehicles=3)
    assert sd.dtype == np.uint32 and list(sd) == [1, 2] and phx.shape == (5,) and list(ghy) == [0, 0, 2, 2, 2]
    assert list(g2) == [np.float32(0.1), np.float32(0.2)] and tries == 4 and delay.dtype == np.int32 and list(delay) == [0, 5, 2]
    assert batch.pack_restart_noise(**ok)[3] is None and batch.pack_restart_noise(**ok)[8] is None
    for bad in (-0.1, np.nan, np.inf, 1.0e6 + 1.0):
        for name in ("pos_box", "goal_box"):
            with pytest.raises(ValueError, match=f"{name} must be finite, >= 0 and <= 1e\\+06 metres"):
                batch.pack_restart_noise(**{**ok, name: np.array([0.5, bad])})
        for name in ("min_gap", "point_gap"):
            with pytest.raises(ValueError, match=f"{name} must be finite, >= 0 and <= 1e\\+06 metres"):
                batch.pack_restart_noise(**ok, **{name: bad})
    for tries in (0, 33, -1, 2.0, True):
        with pytest.raises(ValueError, match="tries must be an integer 1 .. 32"):
            batch.pack_restart_noise(**ok, tries=tries)
    with pytest.raises(ValueError, match="3 entries of pos_box for 2 scenes"):
        batch.pack_restart_noise(**{**ok, "pos_box": [np.zeros(2)] * 3})
    with pytest.raises(ValueError, match="pos_box of shape \\(4, 2\\) for 5 rows"):
        batch.pack_restart_noise(**{**ok, "pos_box": np.zeros((4, 2))})
    with pytest.raises(ValueError, match="seeds: expected a scalar or 2 values"):
        batch.pack_restart_noise(**{**ok, "seeds": [1, 2, 3]})
    with pytest.raises(ValueError, match="seeds must be integers 0 .. 2\\^32-1"):
        batch.pack_restart_noise(**{**ok, "seeds": -1})
    with pytest.raises(ValueError, match="min_gap: expected a scalar or 2 values"):
        batch.pack_restart_noise(**ok, min_gap=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="track_delay must be >= 0 and fit int32"):
        batch.pack_restart_noise(**ok, track_delay=[0, -1, 2], vehicles=3)
    with pytest.raises(ValueError, match="track_delay: expected a scalar or 3 values"):
        batch.pack_restart_noise(**ok, track_delay=[0, 1], vehicles=3)
    with pytest.raises(ValueError, match="track_delay needs the number of device-side vehicles"):
        batch.pack_restart_noise(**ok, track_delay=[0, 1])


def test_entry_points_and_abi():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfm_hip.h")).read(), flags=re.S)
    for name in ("sfm_batch_set_restart_noise", "sfm_batch_download_restart_noise"):
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SYMBOLS and _lib.SINCE[name] == 17
    assert re.search(r"#define SFM_BATCH_PTR_RESETS 6\b", src) and batch.PTR_RESETS == 6
    assert re.search(r"#define SFM_ABI_VERSION 17\b", src) and _lib.ABI_VERSION == 17
    assert len(_lib.SYMBOLS["sfm_batch_set_restart_noise"][1]) == 10
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "sfm_batch_set_restart_noise") and hasattr(raw, "sfm_batch_download_restart_noise")
    assert _lib.load().sfm_abi_version() == 17


def test_the_randomised_example_imports_without_a_gpu():
    spec = importlib.util.spec_from_file_location("batch_rl_loop_randomised", os.path.join(ROOT, "examples", "batch_rl_loop_randomised.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main)
