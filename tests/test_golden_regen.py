"""Generator drift guard: the committed fixtures must be exactly what tests/golden/make_golden.py produces at HEAD.

Round 1 changed scenarios.make_scenario after the fixtures were written, and nothing noticed.  A fixture is the inputs this
project's code builds (scenario, config, waypoint queue) plus the reference's outputs for exactly those inputs; the upstream
checkout is fixed, so the fixture drifts exactly when its inputs do.  This regenerates the inputs of a few cases into a temp
dir with the generator's own case list (``make_golden.py --inputs-only``, no upstream code runs) and compares every array
with the committed file."""
import os
import subprocess
import sys

import numpy as np

import _golden_io as gio

CASES = ["all_s0_n16", "all_s1_n64", "modes_n32", "c1_n64", "coincident_n8", "zspread_n64", "ps_shortrange_rad_n48",
         "ps_integrate_fine_n32"]


def _is_reference_output(key):
    return key.startswith("ref_") or key == "mode_target_speed"


def test_committed_fixtures_are_what_the_generator_writes_today(tmp_path):
    gen = os.path.join(gio.GOLDEN_DIR, "make_golden.py")
    subprocess.check_call([sys.executable, gen, "--inputs-only", "--out", str(tmp_path)] + CASES, stdout=subprocess.DEVNULL)
    for name in CASES:
        new = np.load(tmp_path / (name + ".npz"), allow_pickle=False)
        old = np.load(os.path.join(gio.GOLDEN_DIR, name + ".npz"), allow_pickle=False)
        # every committed key is an input the generator writes today or an output of the reference
        assert sorted(k for k in old.files if not _is_reference_output(k)) == sorted(k for k in new.files if k in old.files), name
        # ... and the one input it may write beyond the committed file is the waypoint queue of a case whose reference v' was
        # not finite (no trajectory was recorded for it)
        for k in set(new.files) - set(old.files):
            assert k == "wp_queue" and "ref_traj_loc" not in old.files and not np.all(np.isfinite(old["ref_new_vel"])), (name, k)
        assert ("wp_queue" in old.files) == ("ref_traj_loc" in old.files), name
        for k in new.files:
            if k not in old.files:
                continue
            a, b = new[k], old[k]
            assert a.dtype == b.dtype and a.shape == b.shape, (name, k)
            assert np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), (name, k)


def test_baseline_c1_fixture_is_the_c1_the_bench_builds():
    """c1_n64.npz must hold the inputs baseline_scenario('c1') builds today (what bench.py --workload c1 runs)."""
    from carla_social_force_model_amd import scenarios
    sc, _ = scenarios.baseline_scenario("c1")
    case = gio.Case(os.path.join(gio.GOLDEN_DIR, "c1_n64.npz"))
    assert np.array_equal(case.loc, sc.loc) and np.array_equal(case.vel, sc.vel)
    for (c0, r0), (c1, r1) in zip(case.dynamic_obstacles, sc.dynamic_obstacles):
        assert np.array_equal(c0, c1) and np.array_equal(r0, r1)
