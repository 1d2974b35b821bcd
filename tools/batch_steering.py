"""Steered pedestrians on a batch (sfm_batch_set_steering, sfm_batch_set_commands, sfm_batch_device_ptr): B = 1024 scenes of 64,
all five forces, 4 moving device-side vehicles per scene.
  --part run     `rounds` rounds of one run(ticks) call of the UNSTEERED batch -- run once per library build (SFM_LIB_PATH names
                 another build) and alternated by tools/batch_steering.sh: this build against its parent
  --part cost    alternated in `rounds` rounds: run(ticks) without steering, and with a quarter of the rows at kind 1 and a quarter
                 at kind 2 (us per tick); medians at the end
  --part step    the RL step, alternated in `rounds` rounds of `ticks` steps each: (s) set_commands + run(1); (t) a write through
                 command_tensor() + run(1); and (u) what a caller had before: state_arrays(), the velocities edited on the host,
                 sfm_batch_upload_state, run(1).  us per step, medians at the end
  --part trace   3 warm-up ticks, run(ticks) on held commands, then `ticks` steps of set_commands + run(1) -- for rocprofv3
                 --kernel-trace --memory-copy-trace: one sfm_batch_tick_kernel launch per tick with no other launch in between,
                 and one host-to-device copy per set_commands step and nothing else
Times are host wall clock around the calls, closed by a device synchronisation."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from carla_social_force_model_amd import scenarios  # noqa: E402
from carla_social_force_model_amd.batch import SfmBatch, pack_scenes  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402

POOL = 32
DT = 0.05
N_B = 64


def _sync():
    import torch
    torch.cuda.synchronize()


def _timed(fn):
    _sync()
    t0 = time.perf_counter()
    fn()
    _sync()
    return time.perf_counter() - t0


class _Setup:
    def __init__(self, B):
        self.B = B
        pool = [vars(scenarios.make_scenario(N_B, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0)))
                for k in range(POOL)]
        self.scenes = [pool[k % POOL] for k in range(B)]
        self.batch = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
        rng = np.random.default_rng(5)
        n = B * N_B
        self.kinds = np.zeros(n, np.uint8)
        order = rng.permutation(n)
        self.kinds[order[:n // 4]] = 1
        self.kinds[order[n // 4:n // 2]] = 2
        self.commands = [np.float32(rng.uniform(-1.2, 1.2, (n, 3))) for _ in range(4)]
        for c in self.commands:
            c[:, 2] = 0.0

    def fresh(self, steer):
        b = self.batch
        b.upload(self.scenes, device_vehicles=True)
        if steer:
            b.set_steering(self.kinds, self.commands[0])
        return b


def _medians(got, base):
    print("# medians (us), and each over the first")
    ref = statistics.median(got[base])
    for name, ts in got.items():
        m = statistics.median(ts)
        print(f"{name:<28} {'med':>5} {m * 1e6:>12.1f} {m / ref:>9.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("run", "cost", "step", "trace"), default="cost")
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    B = 1024
    s = _Setup(B)
    what = f"B = {B} scenes of {N_B}, all five forces, 4 moving device-side vehicles per scene"
    try:
        if args.part == "run":
            print(f"# {args.label}: run({args.ticks}) without steering, {what} "
                  f"({'the build named by SFM_LIB_PATH' if os.environ.get('SFM_LIB_PATH') else 'the in-tree build'})")
            b = s.fresh(False)
            b.run(3)
            for r in range(args.rounds):
                t = _timed(lambda: b.run(args.ticks)) / args.ticks
                print(f"{args.label:<8} {B:>6} {N_B:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
        elif args.part == "cost":
            print(f"# cost of steering: run({args.ticks}), {what}; a quarter of the rows at kind 1, a quarter at kind 2")
            print(f"{'batch':<28} {'round':>5} {'us/tick':>12}")
            got = {"unsteered": [], "steered (1/4 k1, 1/4 k2)": []}
            for r in range(args.rounds):
                for name, steer in zip(got, (False, True)):
                    b = s.fresh(steer)
                    b.run(3)
                    t = _timed(lambda: b.run(args.ticks)) / args.ticks
                    got[name].append(t)
                    print(f"{name:<28} {r:>5} {t * 1e6:>12.1f}", flush=True)
            _medians(got, "unsteered")
        elif args.part == "step":
            import torch
            print(f"# the RL step: {what}; {args.ticks} steps per round, us per step")
            print(f"{'step':<28} {'round':>5} {'us/step':>12}")
            b = s.fresh(True)
            b.set_stream(torch.cuda.current_stream().cuda_stream)
            b.run(3)
            cmd = b.command_tensor()
            dev = [torch.from_numpy(c).to(cmd.device) for c in s.commands]
            pk = pack_scenes(s.scenes)
            L, f = b._lib, (lambda a: np.ascontiguousarray(a, dtype=np.float32))
            steered = s.kinds == 1

            def set_commands():
                for q in range(args.ticks):
                    b.set_commands(s.commands[q % 4])
                    b.run(1)

            def tensor_write():
                for q in range(args.ticks):
                    cmd[:, :3] = dev[q % 4]
                    b.run(1)

            def host_edit():                                           # what a caller had: download, edit, upload, run(1)
                for q in range(args.ticks):
                    loc, vel = b.state_arrays()
                    vel[steered] = s.commands[q % 4][steered]
                    cols = [f(loc[:, 0]), f(loc[:, 1]), f(vel[:, 0]), f(vel[:, 1])]
                    rc = L.sfm_batch_upload_state(b._b, pk["scene_off"].ctypes.data, cols[0].ctypes.data, cols[1].ctypes.data, None,
                                                  cols[2].ctypes.data, cols[3].ctypes.data, None, pk["wx"].ctypes.data,
                                                  pk["wy"].ctypes.data, pk["target_speed"].ctypes.data, pk["radius"].ctypes.data,
                                                  pk["crossing"].ctypes.data)
                    assert rc == 0, L.sfm_batch_last_error(b._b)
                    b.run(1)

            forms = (("s: set_commands + run(1)", set_commands), ("t: tensor write + run(1)", tensor_write))
            got = {n: [] for n, _ in forms}
            got["u: download, edit, upload"] = []
            for r in range(args.rounds):
                for name, fn in forms:
                    t = _timed(fn) / args.ticks
                    got[name].append(t)
                    print(f"{name:<28} {r:>5} {t * 1e6:>12.1f}", flush=True)
            for r in range(args.rounds):                               # (last: the upload drops the steering)
                t = _timed(host_edit) / args.ticks
                got["u: download, edit, upload"].append(t)
                print(f"{'u: download, edit, upload':<28} {r:>5} {t * 1e6:>12.1f}", flush=True)
            _medians(got, "s: set_commands + run(1)")
            assert all(np.isfinite(v).all() for _, v in b.state())
        else:
            b = s.fresh(True)
            b.run(3)
            _sync()
            n = args.ticks

            def steps():
                b.run(n)
                for q in range(n):
                    b.set_commands(s.commands[q % 4])
                    b.run(1)

            t = _timed(steps)
            print(f"# trace: {what}: 3 warm-up ticks, run({n}), then {n} x (set_commands, run(1)) = {2 * n + 3} launches of "
                  f"sfm_batch_tick_kernel and, behind the first of them, {n} host-to-device copies and no other launch expected; "
                  f"{t * 1e6 / (2 * n):.1f} us per tick (wall clock, under the tracer)")
    finally:
        s.batch.close()


if __name__ == "__main__":
    main()
