"""The per-scene argument helpers of ``batch`` and ``scan`` -- ``stream_arrays``, ``mode_scene_arrays``, ``observation_arrays``,
``episode_arrays`` and ``scan.scan_arrays`` -- all check "a scalar or B values" through one function (``_args.per_scene``).  REFUSALS
holds the ValueError text each of them gave, recorded before they shared it, for every argument given in a wrong shape ((3,) for
B = 2, and (2, 2)), a wrong dtype kind, a value that is not finite, a value out of range, and ("both") a wrong shape and a wrong
kind at once: the functions must reproduce each text exactly.  The good path: a scalar, a length-1 array and a length-B array give
equal outputs of the documented dtypes.  Pure NumPy, no GPU."""
import warnings

import numpy as np
import pytest

from carla_social_force_model_amd import batch, scan

B = 2
FUNCS = {   # the function, its good keyword arguments, the dtypes of what it returns (int: a Python int)
    "stream_arrays": (batch.stream_arrays, dict(seeds=7, world_sides=30.0, arrive_thresholds=2.0), (np.uint32, np.float32, np.float32)),
    "mode_scene_arrays": (batch.mode_scene_arrays, dict(despawn_on_arrival=True, sim_time0=0.0, arrive_thresholds=2.0),
                          (np.int32, np.float32, np.float32)),
    "observation_arrays": (batch.observation_arrays, dict(k=4, sense_range=5.0, frame=0), (int, np.float32, int)),
    "episode_arrays": (batch.episode_arrays, dict(agent=0, goal_radius=0.5, ped_radius=0.3, veh_radius=1.0, max_steps=100),
                       (np.int32, np.float32, np.float32, np.float32, np.int32)),
    "scan_arrays": (scan.scan_arrays, dict(max_range=10.0, ped_radius=0.3, point_radius=0.1, frame=0),
                    (np.float32, np.float32, np.float32, int)),
}
NOT_PER_SCENE = ("k", "frame")
VALUES = {  # case -> the bad value (shape cases are built from the argument's good value)
    "kind": {"seeds": 1.5, "agent": 0.5, "max_steps": 1.5, "k": 2.0, "frame": 1.0}, "kind_str": "x", "kind_bool": True,
    "nan": np.nan, "inf": np.inf, "zero": 0.0, "neg": {"agent": -2, "max_steps": -1, None: -1.0},
    "big": {"agent": 1024, "max_steps": 2**31, "k": 17, "frame": 2, None: 2.0e6}, "huge": 1e39,
    "both": {"agent": np.array([0.5, 0.5, 0.5]), None: np.array(["a", "b", "c"])},
}

REFUSALS = [
    ('stream_arrays', 'seeds', 'kind', 'seeds must be integers, got float64'),
    ('stream_arrays', 'seeds', 'kind_str', 'seeds must be integers, got <U1'),
    ('stream_arrays', 'seeds', 'shape3', 'seeds: expected a scalar or 2 values, got shape (3,)'),
    ('stream_arrays', 'seeds', 'shape22', 'seeds: expected a scalar or 2 values, got shape (2, 2)'),
    ('stream_arrays', 'world_sides', 'kind', 'world_sides must be numbers, got <U1'),
    ('stream_arrays', 'world_sides', 'nan', 'world_sides must be finite and >= 0'),
    ('stream_arrays', 'world_sides', 'inf', 'world_sides must be finite and >= 0'),
    ('stream_arrays', 'world_sides', 'neg', 'world_sides must be finite and >= 0'),
    ('stream_arrays', 'world_sides', 'both', 'world_sides: expected a scalar or 2 values, got shape (3,)'),
    ('stream_arrays', 'world_sides', 'shape3', 'world_sides: expected a scalar or 2 values, got shape (3,)'),
    ('stream_arrays', 'world_sides', 'shape22', 'world_sides: expected a scalar or 2 values, got shape (2, 2)'),
    ('stream_arrays', 'arrive_thresholds', 'kind', 'arrive_thresholds must be numbers, got <U1'),
    ('stream_arrays', 'arrive_thresholds', 'nan', 'arrive_thresholds must be finite and >= 0'),
    ('stream_arrays', 'arrive_thresholds', 'neg', 'arrive_thresholds must be finite and >= 0'),
    ('stream_arrays', 'arrive_thresholds', 'shape3', 'arrive_thresholds: expected a scalar or 2 values, got shape (3,)'),
    ('stream_arrays', 'arrive_thresholds', 'shape22', 'arrive_thresholds: expected a scalar or 2 values, got shape (2, 2)'),
    ('mode_scene_arrays', 'despawn_on_arrival', 'kind', 'despawn_on_arrival must be numbers, got <U1'),
    ('mode_scene_arrays', 'despawn_on_arrival', 'shape3', 'despawn_on_arrival: expected a scalar or 2 values, got shape (3,)'),
    ('mode_scene_arrays', 'despawn_on_arrival', 'shape22', 'despawn_on_arrival: expected a scalar or 2 values, got shape (2, 2)'),
    ('mode_scene_arrays', 'sim_time0', 'kind', 'sim_time0 must be numbers, got <U1'),
    ('mode_scene_arrays', 'sim_time0', 'nan', 'sim_time0 must be finite'),
    ('mode_scene_arrays', 'sim_time0', 'inf', 'sim_time0 must be finite'),
    ('mode_scene_arrays', 'sim_time0', 'both', 'sim_time0: expected a scalar or 2 values, got shape (3,)'),
    ('mode_scene_arrays', 'sim_time0', 'shape3', 'sim_time0: expected a scalar or 2 values, got shape (3,)'),
    ('mode_scene_arrays', 'sim_time0', 'shape22', 'sim_time0: expected a scalar or 2 values, got shape (2, 2)'),
    ('mode_scene_arrays', 'arrive_thresholds', 'kind', 'arrive_thresholds must be numbers, got <U1'),
    ('mode_scene_arrays', 'arrive_thresholds', 'nan', 'arrive_thresholds must be finite and >= 0'),
    ('mode_scene_arrays', 'arrive_thresholds', 'neg', 'arrive_thresholds must be finite and >= 0'),
    ('mode_scene_arrays', 'arrive_thresholds', 'shape3', 'arrive_thresholds: expected a scalar or 2 values, got shape (3,)'),
    ('mode_scene_arrays', 'arrive_thresholds', 'shape22', 'arrive_thresholds: expected a scalar or 2 values, got shape (2, 2)'),
    ('observation_arrays', 'sense_range', 'kind', 'sense_range must be numbers, got <U1'),
    ('observation_arrays', 'sense_range', 'kind_bool', 'sense_range must be numbers, got bool'),
    ('observation_arrays', 'sense_range', 'nan', 'sense_range must be finite, > 0 and <= 1e+06 metres'),
    ('observation_arrays', 'sense_range', 'inf', 'sense_range must be finite, > 0 and <= 1e+06 metres'),
    ('observation_arrays', 'sense_range', 'zero', 'sense_range must be finite, > 0 and <= 1e+06 metres'),
    ('observation_arrays', 'sense_range', 'neg', 'sense_range must be finite, > 0 and <= 1e+06 metres'),
    ('observation_arrays', 'sense_range', 'big', 'sense_range must be finite, > 0 and <= 1e+06 metres'),
    ('observation_arrays', 'sense_range', 'huge', 'sense_range must be finite, > 0 and <= 1e+06 metres'),
    ('observation_arrays', 'sense_range', 'both', 'sense_range must be numbers, got <U1'),
    ('observation_arrays', 'sense_range', 'shape3', 'sense_range: expected a scalar or 2 values, got shape (3,)'),
    ('observation_arrays', 'sense_range', 'shape22', 'sense_range: expected a scalar or 2 values, got shape (2, 2)'),
    ('observation_arrays', 'k', 'zero', 'k must be an integer 1 .. 16 (neighbour slots per row), got 0'),
    ('observation_arrays', 'k', 'big', 'k must be an integer 1 .. 16 (neighbour slots per row), got 17'),
    ('observation_arrays', 'k', 'kind', 'k must be an integer 1 .. 16 (neighbour slots per row), got 2.0'),
    ('observation_arrays', 'frame', 'big', "frame must be 0 (world axes) or 1 (the row's heading frame), got 2"),
    ('observation_arrays', 'frame', 'kind', "frame must be 0 (world axes) or 1 (the row's heading frame), got 1.0"),
    ('observation_arrays', 'frame', 'kind_bool', "frame must be 0 (world axes) or 1 (the row's heading frame), got True"),
    ('episode_arrays', 'agent', 'kind', 'agent must be integers, got float64'),
    ('episode_arrays', 'agent', 'neg', 'agent must be -1 (no agent) or a row 0 .. N_b-1 of its scene, got -2 .. -2'),
    ('episode_arrays', 'agent', 'big', 'agent must be -1 (no agent) or a row 0 .. N_b-1 of its scene, got 1024 .. 1024'),
    ('episode_arrays', 'agent', 'both', 'agent must be integers, got float64'),
    ('episode_arrays', 'agent', 'shape3', 'agent: expected a scalar or 2 values, got shape (3,)'),
    ('episode_arrays', 'agent', 'shape22', 'agent: expected a scalar or 2 values, got shape (2, 2)'),
    ('episode_arrays', 'goal_radius', 'kind', 'goal_radius must be numbers, got <U1'),
    ('episode_arrays', 'goal_radius', 'kind_bool', 'goal_radius must be numbers, got bool'),
    ('episode_arrays', 'goal_radius', 'nan', 'goal_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'goal_radius', 'inf', 'goal_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'goal_radius', 'neg', 'goal_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'goal_radius', 'big', 'goal_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'goal_radius', 'huge', 'goal_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'goal_radius', 'shape3', 'goal_radius: expected a scalar or 2 values, got shape (3,)'),
    ('episode_arrays', 'goal_radius', 'shape22', 'goal_radius: expected a scalar or 2 values, got shape (2, 2)'),
    ('episode_arrays', 'ped_radius', 'kind', 'ped_radius must be numbers, got <U1'),
    ('episode_arrays', 'ped_radius', 'nan', 'ped_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'ped_radius', 'neg', 'ped_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'ped_radius', 'big', 'ped_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'ped_radius', 'shape3', 'ped_radius: expected a scalar or 2 values, got shape (3,)'),
    ('episode_arrays', 'ped_radius', 'shape22', 'ped_radius: expected a scalar or 2 values, got shape (2, 2)'),
    ('episode_arrays', 'veh_radius', 'kind', 'veh_radius must be numbers, got <U1'),
    ('episode_arrays', 'veh_radius', 'nan', 'veh_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'veh_radius', 'neg', 'veh_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'veh_radius', 'big', 'veh_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('episode_arrays', 'veh_radius', 'shape3', 'veh_radius: expected a scalar or 2 values, got shape (3,)'),
    ('episode_arrays', 'veh_radius', 'shape22', 'veh_radius: expected a scalar or 2 values, got shape (2, 2)'),
    ('episode_arrays', 'max_steps', 'kind', 'max_steps must be integers, got float64'),
    ('episode_arrays', 'max_steps', 'neg', 'max_steps must be >= 0 (0: no time limit) and fit int32'),
    ('episode_arrays', 'max_steps', 'big', 'max_steps must be >= 0 (0: no time limit) and fit int32'),
    ('episode_arrays', 'max_steps', 'shape3', 'max_steps: expected a scalar or 2 values, got shape (3,)'),
    ('episode_arrays', 'max_steps', 'shape22', 'max_steps: expected a scalar or 2 values, got shape (2, 2)'),
    ('scan_arrays', 'max_range', 'kind', 'max_range must be numbers, got <U1'),
    ('scan_arrays', 'max_range', 'kind_bool', 'max_range must be numbers, got bool'),
    ('scan_arrays', 'max_range', 'nan', 'max_range must be finite, > 0 and <= 1e+06 metres'),
    ('scan_arrays', 'max_range', 'inf', 'max_range must be finite, > 0 and <= 1e+06 metres'),
    ('scan_arrays', 'max_range', 'zero', 'max_range must be finite, > 0 and <= 1e+06 metres'),
    ('scan_arrays', 'max_range', 'neg', 'max_range must be finite, > 0 and <= 1e+06 metres'),
    ('scan_arrays', 'max_range', 'big', 'max_range must be finite, > 0 and <= 1e+06 metres'),
    ('scan_arrays', 'max_range', 'huge', 'max_range must be finite, > 0 and <= 1e+06 metres'),
    ('scan_arrays', 'max_range', 'both', 'max_range must be numbers, got <U1'),
    ('scan_arrays', 'max_range', 'shape3', 'max_range: expected a scalar or 2 values, got shape (3,)'),
    ('scan_arrays', 'max_range', 'shape22', 'max_range: expected a scalar or 2 values, got shape (2, 2)'),
    ('scan_arrays', 'ped_radius', 'kind', 'ped_radius must be numbers, got <U1'),
    ('scan_arrays', 'ped_radius', 'nan', 'ped_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('scan_arrays', 'ped_radius', 'neg', 'ped_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('scan_arrays', 'ped_radius', 'big', 'ped_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('scan_arrays', 'ped_radius', 'shape3', 'ped_radius: expected a scalar or 2 values, got shape (3,)'),
    ('scan_arrays', 'ped_radius', 'shape22', 'ped_radius: expected a scalar or 2 values, got shape (2, 2)'),
    ('scan_arrays', 'point_radius', 'kind', 'point_radius must be numbers, got <U1'),
    ('scan_arrays', 'point_radius', 'nan', 'point_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('scan_arrays', 'point_radius', 'neg', 'point_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('scan_arrays', 'point_radius', 'big', 'point_radius must be finite, >= 0 and <= 1e+06 metres'),
    ('scan_arrays', 'point_radius', 'shape3', 'point_radius: expected a scalar or 2 values, got shape (3,)'),
    ('scan_arrays', 'point_radius', 'shape22', 'point_radius: expected a scalar or 2 values, got shape (2, 2)'),
    ('scan_arrays', 'frame', 'big', "frame must be 0 (world axes) or 1 (the row's heading frame), got 2"),
    ('scan_arrays', 'frame', 'kind', "frame must be 0 (world axes) or 1 (the row's heading frame), got 1.0"),
    ('scan_arrays', 'frame', 'kind_bool', "frame must be 0 (world axes) or 1 (the row's heading frame), got True"),
]


def _bad_value(arg, case, good):
    if case == "shape3":
        return np.full(3, good)
    if case == "shape22":
        return np.full((2, 2), good)
    v = VALUES[case]
    if case == "kind":
        return v.get(arg, "x")
    if case == "zero" and arg == "k":
        return 0
    return v.get(arg, v[None]) if isinstance(v, dict) else v


@pytest.mark.parametrize("fn", sorted(FUNCS))
def test_refusals_keep_their_text(fn):
    f, good, _ = FUNCS[fn]
    cases = [(arg, case, text) for name, arg, case, text in REFUSALS if name == fn]
    assert len(cases) >= 14
    for arg, case, text in cases:
        kw = dict(good)
        kw[arg] = _bad_value(arg, case, good[arg])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                            # (float32 overflow of a value that is then refused)
            with pytest.raises(ValueError) as e:
                f(B, **kw)
        assert str(e.value) == text, (fn, arg, case)


def test_every_per_scene_argument_has_every_kind_of_refusal():
    for fn, (_, good, _) in FUNCS.items():
        for arg in good:
            cases = {case for name, a, case, _ in REFUSALS if name == fn and a == arg}
            if arg in NOT_PER_SCENE:
                assert {"kind", "big"} <= cases, (fn, arg)
            else:
                assert {"shape3", "shape22", "kind"} <= cases, (fn, arg)


@pytest.mark.parametrize("fn", sorted(FUNCS))
def test_scalar_one_value_and_B_values_agree(fn):
    f, good, dtypes = FUNCS[fn]
    as1 = {a: v if a in NOT_PER_SCENE else np.array([v]) for a, v in good.items()}
    asB = {a: v if a in NOT_PER_SCENE else np.array([v] * B) for a, v in good.items()}
    outs = [f(B, **kw) for kw in (good, as1, asB)]
    for out in outs:
        assert len(out) == len(dtypes)
        for o, dt in zip(out, dtypes):
            if dt is int:
                assert type(o) is int
            else:
                assert isinstance(o, np.ndarray) and o.dtype == dt and o.shape == (B,) and o.flags.c_contiguous
    for out in outs[1:]:
        for o, ref in zip(out, outs[0]):
            assert np.array_equal(o, ref)
    # ... and B different values come through in order
    assert np.array_equal(batch.observation_arrays(B, 1, [2.0, 3.0])[1], np.array([2.0, 3.0], np.float32))
    assert np.array_equal(scan.scan_arrays(B, [2.0, 3.0], 0.0, [0.0, 0.5])[2], np.array([0.0, 0.5], np.float32))
    assert np.array_equal(batch.episode_arrays(B, [-1, 5], max_steps=[0, 9])[4], np.array([0, 9], np.int32))
