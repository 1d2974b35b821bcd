"""CPU checks of the batch's pedestrian modes (ABI 9): pack_modes' CSR layout over scenes of 0 / 1 / many pedestrians, plans from
PedModeManager mirrors, broadcast of the per-scene scalars, refused input, and the binding's ABI entries.  No GPU needed."""
import numpy as np
import pytest

from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import MODE_KEYS, mode_scene_arrays, pack_modes, plan_from_managers
from carla_social_force_model_amd.ped_mode_manager import PedMode, PedModeManager


def _plan(n, seed, queue_lens=None):
    rng = np.random.default_rng(seed)
    lens = queue_lens if queue_lens is not None else rng.integers(0, 4, n)
    return {"mode": rng.integers(0, 5, n), "target_speed": rng.uniform(0.0, 2.0, n), "initial_speed": rng.uniform(1.0, 1.5, n),
            "crossing_speed": rng.uniform(1.5, 2.0, n), "safety_margin": rng.uniform(-1.0, 2.0, n),
            "next_mode_time": rng.uniform(-1.0, 6.0, n),
            "queues": [[(rng.uniform(-9, 9, 3), bool(rng.integers(0, 2))) for _ in range(int(lens[i]))] for i in range(n)]}


def test_pack_modes_csr_across_scenes():
    sizes = [0, 1, 5, 0, 3]
    scene_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    plans = [_plan(n, 10 + k) for k, n in enumerate(sizes)]
    plans[2]["first_vehicle_extent"] = (2.5, 1.0)
    scenes = [{"dynamic_extent": None}, {"dynamic_extent": np.array([[1.5, 0.75], [9.0, 9.0]])}, {}, {"dynamic_extent": []}, {}]
    pm = pack_modes(plans, scene_off, scenes)
    N = int(scene_off[-1])
    assert pm["mode"].dtype == np.uint8 and pm["mode"].shape == (N,)
    for k in MODE_KEYS[1:]:
        assert pm[k].dtype == np.float32 and pm[k].shape == (N,) and pm[k].flags["C_CONTIGUOUS"]
    assert pm["wp_offsets"].dtype == np.int32 and pm["wp_offsets"].shape == (N + 1,) and pm["wp_offsets"][0] == 0
    assert pm["first_vehicle_extent"].shape == (5, 2) and pm["first_vehicle_extent"].dtype == np.float32
    assert pm["first_vehicle_extent"].tolist() == [[0, 0], [1.5, 0.75], [2.5, 1.0], [0, 0], [0, 0]]
    # every row in concatenated scene order, its queue at wp_offsets[row] .. wp_offsets[row+1]
    row = 0
    for k, plan in enumerate(plans):
        for i in range(sizes[k]):
            assert pm["mode"][row] == plan["mode"][i]
            for key in MODE_KEYS[1:]:
                assert pm[key][row] == np.float32(plan[key][i]), (k, i, key)
            q = plan["queues"][i]
            e0, e1 = pm["wp_offsets"][row], pm["wp_offsets"][row + 1]
            assert e1 - e0 == len(q)
            for e, (w, cross) in zip(range(e0, e1), q):
                assert pm["wp_x"][e] == np.float32(w[0]) and pm["wp_y"][e] == np.float32(w[1])
                assert pm["wp_crossing"][e] == int(cross)
            row += 1
    assert row == N and pm["wp_x"].shape == pm["wp_crossing"].shape == (int(pm["wp_offsets"][-1]),)
    # no scenes dicts: zeros unless the plan says otherwise
    assert pack_modes(plans, scene_off)["first_vehicle_extent"].tolist() == [[0, 0], [0, 0], [2.5, 1.0], [0, 0], [0, 0]]


def test_pack_modes_all_empty():
    pm = pack_modes([_plan(0, 1), _plan(0, 2)], np.zeros(3, np.int32))
    assert pm["mode"].shape == (0,) and pm["wp_offsets"].tolist() == [0] and pm["wp_x"].shape == (0,)


def test_plan_from_managers_matches_the_explicit_plan():
    ms = []
    for i in range(7):
        m = PedModeManager(f"p{i}", 1.0 + 0.1 * i, PedMode.WALKING_SIDEWALK, 1.5, -1.0 if i % 3 == 0 else 0.5)
        if i == 2:
            m.set_mode(PedMode.IDLE)
        if i == 4:
            m.set_mode(PedMode.CROSSING_ROAD)            # diverted to CHECKING_TRAFFIC
        ms.append(m)
    queues = [[(np.array([i, -i, 0.0]), bool(i % 2))] * (i % 3) for i in range(7)]
    explicit = {"mode": [int(m.current_mode) for m in ms], "target_speed": [m.target_speed for m in ms],
                "initial_speed": [m.initial_target_speed for m in ms], "crossing_speed": [m.crossing_speed for m in ms],
                "safety_margin": [m.crossing_safety_margin for m in ms], "next_mode_time": [m.next_mode_time for m in ms],
                "queues": queues}
    assert explicit["mode"][2] == int(PedMode.IDLE) and explicit["mode"][4] == int(PedMode.CHECKING_TRAFFIC)
    so = np.array([0, 3, 7], np.int32)
    a = pack_modes([plan_from_managers(ms[:3], queues[:3]), plan_from_managers(ms[3:], queues[3:])], so)
    b = pack_modes([{k: (v[:3] if k != "queues" else v[:3]) for k, v in explicit.items()},
                    {k: v[3:] for k, v in explicit.items()}], so)
    for key in a:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key


def test_make_mode_plan_follows_the_recipe():
    sc = vars(scenarios.make_scenario(30, 5, n_dynamic=2))
    wp0 = sc["waypoint"].copy()
    plan, ms = scenarios.make_mode_plan(sc, 9, queue_len=2)
    assert len(ms) == 30 and len(plan["queues"]) == 30 and all(len(q) == 2 for q in plan["queues"])
    assert [int(m) for m in plan["mode"]] == [int(PedMode.IDLE) if i % 11 == 3 else int(PedMode.WALKING_SIDEWALK) for i in range(30)]
    assert all((plan["safety_margin"][i] < 0) == (i % 5 == 0) for i in range(30))
    assert np.all(np.abs(sc["waypoint"][:, :2] - sc["loc"][:, :2]) <= 3.0 + 1e-6)
    assert not np.array_equal(sc["waypoint"], wp0)
    pm = pack_modes([plan], np.array([0, 30], np.int32), [sc])
    assert pm["first_vehicle_extent"][0].tolist() == np.float32(sc["dynamic_extent"][0]).tolist()


def test_scene_scalars_broadcast():
    d, t, r = mode_scene_arrays(3, True, 1.5, 2.0)
    assert d.dtype == np.int32 and d.tolist() == [1, 1, 1]
    assert t.dtype == np.float32 and t.tolist() == [1.5] * 3 and r.tolist() == [2.0] * 3
    d, t, r = mode_scene_arrays(3, [1, 0, 1], [0.0, 0.25, 0.5], [1.0])
    assert d.tolist() == [1, 0, 1] and t.tolist() == [0.0, 0.25, 0.5] and r.tolist() == [1.0] * 3
    for c in (d, t, r):
        assert c.flags["C_CONTIGUOUS"] and c.shape == (3,)


@pytest.mark.parametrize("args, msg", [
    (dict(despawn_on_arrival=[1, 0]), "despawn_on_arrival"),
    (dict(sim_time0=np.inf), "sim_time0"),
    (dict(sim_time0=[0.0, np.nan, 0.0]), "sim_time0"),
    (dict(arrive_thresholds=-1.0), "arrive_thresholds"),
    (dict(arrive_thresholds=[1.0, np.inf, 1.0]), "arrive_thresholds"),
    (dict(arrive_thresholds=np.ones((3, 1))), "arrive_thresholds"),
    (dict(sim_time0="soon"), "sim_time0"),
])
def test_scene_scalars_refused(args, msg):
    with pytest.raises(ValueError, match=msg):
        mode_scene_arrays(3, **args)


def _bad(edit):
    plans = [_plan(2, 1, [1, 2]), _plan(3, 2, [0, 1, 2])]
    edit(plans[1])
    return plans


@pytest.mark.parametrize("edit, msg", [
    (lambda p: p.pop("initial_speed"), "scene 1: the mode plan has no initial_speed"),
    (lambda p: p.pop("queues"), "scene 1: the mode plan has no queues"),
    (lambda p: p.update(mode=[1, 2, 7]), "scene 1: mode must hold PedMode values"),
    (lambda p: p.update(mode=[1, 2, -1]), "scene 1: mode must hold PedMode values"),
    (lambda p: p.update(mode=[1, 2.5, 1]), "scene 1: mode must hold PedMode values"),
    (lambda p: p.update(target_speed=[1.0, 1.0]), "scene 1: target_speed has 2 rows, expected 3"),
    (lambda p: p.update(next_mode_time=np.zeros(4)), "scene 1: next_mode_time has 4 rows, expected 3"),
    (lambda p: p.update(queues=[[], []]), "scene 1: queues has 2 lists, expected 3"),
    (lambda p: p.update(queues=[[], [(np.zeros(3),)], []]), r"scene 1: queues\[1\]\[0\] must be a \(waypoint, crossing_road\) pair"),
    (lambda p: p.update(queues=[[], [(np.zeros(4), True)], []]), r"scene 1: queues\[1\]\[0\] has a waypoint of 4 coordinates"),
    (lambda p: p.update(first_vehicle_extent=(1.0, 2.0, 3.0)), "scene 1: first_vehicle_extent must have 2 values"),
])
def test_pack_modes_refusals(edit, msg):
    with pytest.raises(ValueError, match=msg):
        pack_modes(_bad(edit), np.array([0, 2, 5], np.int32))


def test_pack_modes_counts_refused():
    with pytest.raises(ValueError, match="1 mode plans for 2 scenes"):
        pack_modes([_plan(2, 1)], np.array([0, 2, 5], np.int32))
    with pytest.raises(ValueError, match="scene 0: a mode plan must be a dict"):
        pack_modes([[1, 2], _plan(3, 2)], np.array([0, 2, 5], np.int32))
    with pytest.raises(ValueError, match="1 scenes for 2 mode plans"):
        pack_modes([_plan(2, 1), _plan(3, 2)], np.array([0, 2, 5], np.int32), [{}])


def test_abi_9_entries():
    assert _lib.ABI_VERSION >= 9
    for name in ("sfm_batch_set_mode_fsm", "sfm_batch_download_modes"):
        assert name in _lib.SYMBOLS and _lib.SINCE[name] == 9, name
    assert len(_lib.SYMBOLS["sfm_batch_set_mode_fsm"][1]) == 15
    assert len(_lib.SYMBOLS["sfm_batch_download_modes"][1]) == 5
