"""Host-side tests of the batch's spawn schedule (no GPU): the PedSpawner mirror against traces of the reference's own class
(tests/golden/spawn/spawn_schedule.npz, written by tests/golden/make_golden_spawn.py), the expansion of spawners into rows with the
NumPy twin of the kernel's birth rule against the same traces (the test of the ``chain`` design), the packer and its refusals, and
the ABI 11 entries in header and binding."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _golden_io as gio
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import pack_modes, pack_spawns
from carla_social_force_model_amd.host_state import PedMode, PedModeManager
from carla_social_force_model_amd.spawner import MODE_UNBORN, PedSpawner, birth_ticks, births, release_times, scene_from_spawners

FIXTURE = os.path.join(gio.GOLDEN_DIR, "spawn", "spawn_schedule.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    d = np.load(FIXTURE, allow_pickle=False)
    out = []
    for k in range(len(d["in_ticks"])):
        w = d["in_wp"][d["in_wp_off"][k]:d["in_wp_off"][k + 1]]
        bools = [bool(x) for x in d["in_cross"][d["in_wp_off"][k]:d["in_wp_off"][k + 1]]]
        speed, qty, t0, interval, factor, margin, dt, clock0 = (float(x) for x in d["in_scalars"][k])
        make = lambda w=w, bools=bools, k=k, a=(speed, None, int(qty), t0, interval, factor, margin): PedSpawner(
            d["in_loc"][k].copy(), w[0].copy() if d["in_flat"][k] else w.copy(), bools, a[0], *a[1:])
        out.append((k, make, dt, clock0, int(d["in_ticks"][k])))
    return d, out


def test_the_fixture_covers_the_cases_the_schedule_has_to_handle():
    d, cases = _cases()
    s = d["in_scalars"]
    assert (s[:, 3] > s[:, 6]).any() and (s[:, 3] < s[:, 6]).any() and (s[:, 3] == s[:, 6]).any()     # interval above / below / at dt
    assert (s[:, 2] < s[:, 7]).any()                                                                # behind the clock
    first = d["in_cross"][d["in_wp_off"][:-1]]
    assert first.any() and not first.all() and d["in_flat"].any()
    k = int(np.nonzero(s[:, 3] < s[:, 6])[0][0])                     # below the step length: the reference releases one per tick
    ticks = np.nonzero(d["ref_release"][k])[0]
    assert len(ticks) == int(s[k, 1]) and (np.diff(ticks) == 1).all()


def test_the_mirror_is_the_reference_spawner():
    d, cases = _cases()
    for k, make, dt, clock0, ticks in cases:
        sp = make()
        assert int(sp.initial_mode) == d["ref_initial_mode"][k], k
        now = np.float32(clock0)
        for t in range(ticks):
            released = sp.quantity > 0 and sp.ready_to_spawn(float(now))
            if released:
                sp.quantity -= 1
            assert int(released) == d["ref_release"][k, t], f"case {k} tick {t}"
            assert abs(sp.next_spawn_time - d["ref_next_spawn_time"][k, t]) <= 1e-12, f"case {k} tick {t}"
            now = np.float32(now + np.float32(dt))
        state, rem = sp.generate_ped_state(f"ped_{k}", 100 + k, 0.25 + 0.05 * k)
        name, cid, loc, vel, wp, mode, radius, speed = state
        assert (name, cid) == (f"ped_{k}", 100 + k) and np.array_equal(loc, d["in_loc"][k])
        assert np.abs(vel - d["ref_velocity"][k]).max() <= 1e-12 and np.array_equal(wp, d["ref_first_waypoint"][k]), k
        assert radius == d["ref_radius"][k] and speed == d["ref_target_speed"][k]
        assert isinstance(mode, PedModeManager)
        got = (int(mode.current_mode), mode.target_speed, mode.crossing_speed, mode.crossing_safety_margin)
        assert got[0] == int(d["ref_mode"][k, 0]) and np.abs(np.array(got[1:]) - d["ref_mode"][k, 1:]).max() <= 1e-12, k
        r0, r1 = d["ref_rem_off"][k], d["ref_rem_off"][k + 1]
        assert len(rem) == r1 - r0
        for (w, c), rw, rc in zip(rem, d["ref_rem_wp"][r0:r1], d["ref_rem_cross"][r0:r1]):
            assert np.array_equal(np.asarray(w), rw) and bool(c) == bool(rc)


def test_the_committed_inputs_are_what_the_generator_writes_today(tmp_path):
    gen = os.path.join(gio.GOLDEN_DIR, "make_golden_spawn.py")
    subprocess.check_call([sys.executable, gen, "--inputs-only", "--out", str(tmp_path)], stdout=subprocess.DEVNULL)
    new, old = np.load(tmp_path / "spawn_schedule.npz", allow_pickle=False), np.load(FIXTURE, allow_pickle=False)
    assert sorted(new.files) == sorted(k for k in old.files if k.startswith("in_")) and len(old.files) > len(new.files)
    for k in new.files:
        assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k


def test_rows_with_chains_are_born_when_the_reference_releases_them():
    """scene_from_spawners + the NumPy twin of the kernel's birth rule against the reference's release ticks, one spawner per scene and
    all of them in one scene (with a pedestrian who is there from the start in front), backlog cases included."""
    d, cases = _cases()
    for k, make, dt, clock0, ticks in cases:
        sp = make()
        scene, plan, sched, managers = scene_from_spawners([sp], radius=0.3)
        n = sp.quantity
        assert scene["loc"].shape == (n, 3) and len(managers) == n and sp.next_spawn_time == d["in_scalars"][k, 2]      # not advanced
        assert sched["spawn_time"].dtype == np.float32 and sched["chain"].tolist() == [0] + [1] * (n - 1)
        assert np.array_equal(sched["spawn_time"], release_times(sp).astype(np.float32))
        tick, when = birth_ticks(sched["spawn_time"], sched["chain"], clock0, dt, ticks)
        want = np.nonzero(d["ref_release"][k, :ticks])[0]
        assert np.array_equal(tick[:len(want)], want) and (tick[len(want):] == ticks).all(), f"case {k}: {tick} vs {want}"
        assert np.array_equal(np.isnan(when), tick == ticks)
        # the rows are the spawn state: location, velocity, first waypoint, mode plan, queue
        assert np.array_equal(scene["loc"], np.tile(d["in_loc"][k], (n, 1)))
        assert np.abs(scene["vel"] - d["ref_velocity"][k]).max() <= 1e-12
        assert np.array_equal(scene["waypoint"], np.tile(d["ref_first_waypoint"][k], (n, 1)))
        assert (plan["mode"] == d["ref_initial_mode"][k]).all() and len(plan["queues"][0]) == d["ref_rem_off"][k + 1] - d["ref_rem_off"][k]
        pack_modes([plan], np.array([0, n]))                          # ... in the form set_modes takes
    # same clock for all: the spawners that share dt = 0.05 and clock0 = 0 in one scene, behind a pedestrian already there
    same = [c for c in cases if c[2] == 0.05 and c[3] == 0.0]
    assert len(same) >= 3
    sps = [c[1]() for c in same]
    there = PedSpawner(np.zeros(3), np.array([3.0, 0.0, 0.0]), [False], 1.0, None, 1, 0.0, 1.0, 1.5, 1.5).generate_ped_state("p", 0, 0.3)
    scene, plan, sched, _ = scene_from_spawners(sps, radius=[0.3] * len(sps), present=[there[0]], present_queues=[there[1]])
    assert sched["spawn_time"][0] == -np.inf and sched["chain"][0] == 0 and scene["loc"].shape[0] == 1 + sum(s.quantity for s in sps)
    T = min(c[4] for c in same)
    tick, _ = birth_ticks(sched["spawn_time"], sched["chain"], 0.0, 0.05, T)
    assert tick[0] == 0
    o = 1
    for (k, _, _, _, _), sp in zip(same, sps):
        want = np.nonzero(d["ref_release"][k, :T])[0]
        assert np.array_equal(tick[o:o + len(want)], want) and (tick[o + len(want):o + sp.quantity] == T).all(), k
        o += sp.quantity


def test_birth_rule_twin():
    st = np.float32([-np.inf, 0.0, 0.0, 0.0, 5.0, np.inf])
    ch = np.array([0, 0, 1, 1, 0, 0])
    b0 = births(np.zeros(6, bool), st, ch, 0.0)
    assert b0.tolist() == [True, True, False, False, False, False]
    b1 = births(b0, st, ch, 0.05)
    assert b1.tolist() == [True, True, True, False, False, False]          # one per chain per tick
    assert births(b1, st, ch, 5.0).tolist() == [True, True, True, True, True, False]
    assert births(b1, st, ch, np.float32(5.0) - np.float32(1e-6)).tolist() == [True, True, True, True, False, False]
    with pytest.raises(ValueError, match="first row"):
        births(np.zeros(2, bool), [0, 0], [1, 0], 0.0)
    with pytest.raises(ValueError, match="differ in length"):
        births(np.zeros(2, bool), [0, 0, 0], [0, 0], 0.0)
    assert births(np.zeros(0, bool), [], [], 1.0).shape == (0,)
    assert MODE_UNBORN == 254


def test_make_spawn_plan_has_the_cases():
    sc = vars(scenarios.make_scenario(64, 3))
    s = scenarios.make_spawn_plan(sc, 7, dt=0.05, t0=1.0)
    t, c = s["spawn_time"], s["chain"]
    assert t.dtype == np.float32 and c.dtype == np.uint8 and t.shape == c.shape == (64,)
    assert np.isinf(t[:22]).all() and (t[:22] < 0).all() and not c[:23].any()
    assert t[22] < 1.0 and c[23] == 1                                       # a spawner that starts behind the clock
    heads = np.nonzero((c == 0) & np.isfinite(t))[0]
    assert len(heads) == 4
    gaps = [float(t[h + 2] - t[h + 1]) for h in heads]
    assert min(gaps) < 0.05 < max(gaps)                                     # intervals below and above the step length
    assert np.array_equal(scenarios.make_spawn_plan(sc, 7, dt=0.05, t0=1.0)["spawn_time"], t)
    nobody = scenarios.make_spawn_plan(sc, 7, dt=0.05, t0=1.0, present=0.0)
    assert np.isfinite(nobody["spawn_time"]).all() and (nobody["spawn_time"] > 1.0).all()
    pack_spawns([s, None, nobody], [0, 64, 64, 128])


def test_pack_spawns():
    so = np.array([0, 3, 3, 5, 7], np.int32)
    t, c = pack_spawns([{"spawn_time": [0.5, -np.inf, np.inf], "chain": [0, 1, 0]}, {"spawn_time": []}, None,
                        {"spawn_time": np.array([1.0, 1.1]), "chain": None}], so)
    assert t.dtype == np.float32 and c.dtype == np.uint8
    assert np.array_equal(t, np.float32([0.5, -np.inf, np.inf, -np.inf, -np.inf, 1.0, 1.1])) and c.tolist() == [0, 1, 0, 0, 0, 0, 0]
    t, c = pack_spawns([None], [0, 0])
    assert t.shape == (0,) and c.shape == (0,)
    ok = {"spawn_time": [0.0, 1.0, 2.0], "chain": [0, 1, 1]}
    for bad, msg in (([ok], "1 spawn schedules for 4 scenes"),
                     ([ok, None, None, 5], "scene 3: a spawn schedule must be a dict or None"),
                     ([{"chain": [0, 0, 0]}, None, None, None], "scene 0: the spawn schedule has no spawn_time"),
                     ([{"spawn_time": [0.0, 1.0]}, None, None, None], "scene 0: spawn_time has 2 rows, expected 3"),
                     ([ok, None, {"spawn_time": [0, 0], "chain": [0]}, None], "scene 2: chain has 1 rows, expected 2"),
                     ([{"spawn_time": [0.0, np.nan, 2.0]}, None, None, None], "scene 0: spawn_time must not be NaN"),
                     ([{"spawn_time": [0, 0, 0], "chain": [0, 2, 0]}, None, None, None], "scene 0: chain must hold 0 or 1"),
                     ([ok, None, {"spawn_time": [0, 0], "chain": [1, 0]}, None], "scene 2: chain must be 0 on the scene's first row")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            pack_spawns(bad, so)


def test_abi_version_carries_the_spawn_schedule():
    assert _lib.ABI_VERSION >= 11
    header = open(os.path.join(ROOT, "include", "sfm_hip.h")).read()
    assert int(re.search(r"#define SFM_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    assert re.search(r"#define SFM_MODE_UNBORN 254\b", header)
    for name, nargs in (("sfm_batch_set_spawn_schedule", 3), ("sfm_batch_download_spawns", 3)):
        assert re.search(r"\bint " + name + r"\(SfmBatch\* b,", header), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs and _lib.SINCE[name] == 11
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.sfm_batch_set_spawn_schedule and lib.sfm_batch_download_spawns
