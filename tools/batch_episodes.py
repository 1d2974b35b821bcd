"""Episode ends and the restart by device mask on a batch (sfm_batch_set_episodes, sfm_batch_end_step, sfm_batch_restart_device):
B = 1024 scenes of 64, all five forces, 4 moving device-side vehicles per scene.
  --part run     `rounds` rounds of one run(ticks) call of the batch WITHOUT episodes -- run once per library build
                 (SFM_LIB_PATH names another build) and alternated by tools/batch_episodes.sh: this build against its parent
  --part ep      alternated in `rounds` rounds of `ticks` calls each (us per call, medians at the end):
                 (a) end_step() beside observe() (K = 4) and one tick launch (run(1)) of the same batch;
                 (c) restart_device() with 1/8 of the scenes chosen against restart(mask) with the same mask
  --part loop    one step of examples/batch_rl_loop.py (the host decides who is done: a device-to-host copy and a host-mask restart
                 per step) against one of examples/batch_rl_loop_device.py (end_step(auto_restart=True)), alternated in `rounds`
                 rounds of --steps steps at --scenes / --repeat.  The loop alone is timed: from the return of the example's
                 snapshot() (after a device synchronisation) to its close() (after another)
  --part trace   the loop of --example (host | device), --steps steps -- for rocprofv3 --kernel-trace --memory-copy-trace: the
                 launches and copies per step
Times are host wall clock around the calls, closed by a device synchronisation."""
from __future__ import annotations

import argparse
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from carla_social_force_model_amd import scenarios  # noqa: E402
from carla_social_force_model_amd.batch import SfmBatch  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402

POOL = 32
DT = 0.05
N_B = 64
K = 4
RANGE = 5.0


def _sync():
    import torch
    torch.cuda.synchronize()


def _timed(fn):
    _sync()
    t0 = time.perf_counter()
    fn()
    _sync()
    return time.perf_counter() - t0


def _batch(B):
    pool = [vars(scenarios.make_scenario(N_B, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0))) for k in range(POOL)]
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    b.upload([pool[k % POOL] for k in range(B)], device_vehicles=True)
    return b


def _medians(got, base):
    print("# medians (us), and each over the first")
    ref = statistics.median(got[base])
    for name, ts in got.items():
        m = statistics.median(ts)
        print(f"{name:<52} {'med':>5} {m * 1e6:>12.1f} {m / ref:>9.2f}x")


def _example(which):
    name = "batch_rl_loop" if which == "host" else "batch_rl_loop_device"
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def _loop_seconds(ex, B, steps, repeat):
    """Seconds the example's loop takes: the clock starts when its snapshot() returns and stops when its close() is called, a device
    synchronisation in front of each reading.  (Both examples take the snapshot last before the loop and close the batch first after.)"""
    mark = {}
    snapshot, close = SfmBatch.snapshot, SfmBatch.close

    def snap(self):
        snapshot(self)
        _sync()
        mark["t0"] = time.perf_counter()

    def shut(self):
        if "t1" not in mark:
            _sync()
            mark["t1"] = time.perf_counter()
        close(self)

    SfmBatch.snapshot, SfmBatch.close = snap, shut
    try:
        ended = ex.run(B=B, steps=steps, repeat=repeat, quiet=True)
    finally:
        SfmBatch.snapshot, SfmBatch.close = snapshot, close
    return mark["t1"] - mark["t0"], ended


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("run", "ep", "loop", "trace"), default="ep")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=4)
    ap.add_argument("--example", choices=("host", "device"), default="device")
    args = ap.parse_args()
    B = args.scenes
    what = f"B = {B} scenes of {N_B}, all five forces, 4 moving device-side vehicles per scene"
    batches = []
    try:
        if args.part == "run":
            print(f"# {args.label}: run({args.ticks}) without episodes, {what} "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            b = _batch(B)
            batches.append(b)
            b.run(3)
            for r in range(args.rounds):
                t = _timed(lambda: b.run(args.ticks)) / args.ticks
                print(f"{args.label:<8} {B:>6} {N_B:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
        elif args.part == "ep":
            import torch
            print(f"# episodes: {what}; agent row 0, radii 1.0 / 0.3 / 0.3 m, no time limit; {args.ticks} calls per round, us per call")
            print(f"{'form':<52} {'round':>5} {'us/call':>12}")
            b = _batch(B)
            batches.append(b)
            b.set_stream(torch.cuda.current_stream().cuda_stream)
            b.set_observation(K, RANGE)
            b.set_episodes(0, 1.0, 0.3, 0.3, 0)
            b.run(3)
            b.snapshot()
            mask = np.zeros(B, bool)
            mask[::8] = True
            d_mask = torch.from_numpy(mask).cuda()

            def repeat(fn):
                def go():
                    for _ in range(args.ticks):
                        fn()
                return go

            forms = (("a: end_step()", repeat(b.end_step)),
                     ("a: observe(), K = 4", repeat(b.observe)),
                     ("a: run(1), one tick launch", repeat(lambda: b.run(1))),
                     ("a: end_step(auto_restart=True)", repeat(lambda: b.end_step(auto_restart=True))),
                     ("c: restart_device(mask on the device), 1/8 chosen", repeat(lambda: b.restart_device(d_mask))),
                     ("c: restart(mask on the host), the same mask", repeat(lambda: b.restart(mask))))
            got = {n: [] for n, _ in forms}
            for _, fn in forms:                                        # warm-up: the first launches, the pinned list
                fn()
            for r in range(args.rounds):
                for name, fn in forms:
                    t = _timed(fn) / args.ticks
                    got[name].append(t)
                    print(f"{name:<52} {r:>5} {t * 1e6:>12.1f}", flush=True)
            _medians(got, "a: end_step()")
        elif args.part == "loop":
            print(f"# loop: {B} scenes of {N_B}, {args.steps} steps of {args.repeat} ticks per round; us per loop step")
            print(f"{'example':<52} {'round':>5} {'us/step':>12}   (episodes ended, of them at the goal)")
            names = {"host": "b: examples/batch_rl_loop.py (host mask)", "device": "b: examples/batch_rl_loop_device.py (no host)"}
            exs = {w: _example(w) for w in names}
            got = {n: [] for n in names.values()}
            for w in names:                                            # warm-up: torch's allocator and kernels, the first launches
                _loop_seconds(exs[w], B, 10, args.repeat)
            for r in range(args.rounds):
                for w, name in names.items():
                    t, ended = _loop_seconds(exs[w], B, args.steps, args.repeat)
                    got[name].append(t / args.steps)
                    print(f"{name:<52} {r:>5} {t / args.steps * 1e6:>12.1f}   {ended}", flush=True)
            _medians(got, names["host"])
        else:
            ex = _example(args.example)
            t, ended = _loop_seconds(ex, B, args.steps, args.repeat)
            print(f"# trace: examples/{ex.__name__}.py, {B} scenes of {N_B}, {args.steps} steps of {args.repeat} ticks: "
                  f"{t / args.steps * 1e6:.1f} us per step (wall clock, under the tracer); episodes ended {ended}")
    finally:
        for b in batches:
            b.close()


if __name__ == "__main__":
    main()
