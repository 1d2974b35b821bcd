"""Scene-ticks per second of batched scenes (SfmBatch: one launch per tick for the whole batch) against one SfmEngine handle per
scene.  One part per call, so that tools/batch_throughput.sh can run each under its own time limit:

  --part batch     B in {64, 1024, 8192} scenes of N_b in {20, 64, 256}: pedestrian + acceleration forces, then all five forces
                   with 40 border points (two borders of 20) and 4 obstacles (2 static, 2 vehicles) per scene
  --part handles   the same scenes on B separate handles stepped with run(1) in a loop, B in {64, 1024}, N_b = 64
  --part trace     B = 1024, N_b = 64, pedestrian + acceleration: a fixed number of batch ticks, for rocprofv3 --kernel-trace --stats
  --part streams   B in {1024, 8192} scenes of 64, pedestrian + acceleration: run(K), run(K, redraw=True) (per-scene waypoint
                   streams), run_recorded(K, stride=1) (every tick a frame, one device-to-host copy at the end, included in the
                   time) and, for comparison, the same trajectory taken step-wise (state_arrays() + run(1) per tick), alternated
  --part plain     the run(K) rows of `streams` only, with the library SFM_LIB_PATH names (A/B of builds: ABI 6 has no streams)
  --part trace-recorded   B = 1024, N_b = 64: 3 warm-up ticks, then run_recorded(K, stride=1) -- for rocprofv3: K launches of the
                   recording kernel, one per tick
  --part vehicles  B = 1024 scenes of 64, all five forces, 4 vehicles per scene (2 borders, 2 static obstacles), three forms
                   alternated: (a) rings set once and never moved, (b) device-side vehicles (upload(device_vehicles=True)) moving
                   inside the tick's launch, (c) moving traffic without them -- the host twin advanced in NumPy (vectorised over every
                   vehicle, the device's fp32 arithmetic) and sfm_batch_set_dynamic_obstacles before every run(1)
  --part rings     the batch without device-side vehicles, for an A/B of builds (SFM_LIB_PATH): form (a) of `vehicles`, and the
                   all-five-forces row of `batch` at B = 1024, N_b = 64 (2 borders of 20 points, 2 static obstacles, 2 vehicles)
  --part trace-vehicles   form (b) alone: one set_dynamic_boxes, 3 warm-up ticks, run(K) -- for rocprofv3: K + 3 launches of
                   sfm_batch_tick_kernel and one of sfm_dynamic_boxes_kernel

Times are host wall clock around K back-to-back ticks after a warm-up, closed by a device synchronisation (the work is issued on
the null stream).  A pool of distinct scenes is generated once per shape and repeated to fill the batch.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from carla_social_force_model_amd import scenarios  # noqa: E402
from carla_social_force_model_amd._lib import fptr, iptr  # noqa: E402
from carla_social_force_model_amd.batch import SfmBatch, pack_boxes, pack_scenes  # noqa: E402
from carla_social_force_model_amd.config import default_sfm_config  # noqa: E402
from carla_social_force_model_amd.engine import SfmEngine  # noqa: E402

PED = ("acceleration_force", "pedestrian_force")
POOL = 32


def _pool(n, geo):
    kw = dict(n_borders=2, n_static=2, n_dynamic=2, border_len=(2.0, 2.0)) if geo else {}
    return [vars(scenarios.make_scenario(n, 7000 + k, **kw)) for k in range(POOL)]


def _sync():
    import torch
    torch.cuda.synchronize()


def _time_batch(B, n, geo, ticks):
    pool = _pool(n, geo)
    scenes = [pool[k % POOL] for k in range(B)]
    cfg = default_sfm_config(scenarios.ALL_FORCES if geo else PED)
    b = SfmBatch(cfg, 0.05, B=B)
    try:
        b.upload_packed(pack_scenes(scenes))
        b.run(3)
        _sync()
        t0 = time.perf_counter()
        b.run(ticks)
        _sync()
        dt = time.perf_counter() - t0
        assert all(np.isfinite(v).all() for _, v in b.state()[:POOL])
    finally:
        b.close()
    return dt / ticks


def _streams_batch(B, n):
    pool = _pool(n, False)
    b = SfmBatch(default_sfm_config(PED), 0.05, B=B)
    b.upload_packed(pack_scenes([pool[k % POOL] for k in range(B)]))
    return b, [pool[k % POOL]["world_side"] for k in range(B)]


def _time_mode(b, mode, ticks):
    """Seconds per tick of one call of `mode` (plain / redraw / recorded) after a 3-tick warm-up of the same kind."""
    def stepwise(k):
        for _ in range(k):
            b.state_arrays()
            b.run(1)
    call = {"plain": lambda k: b.run(k), "redraw": lambda k: b.run(k, redraw=True),
            "recorded": lambda k: b.run_recorded(k, stride=1), "stepwise": stepwise}[mode]
    call(3)
    _sync()
    t0 = time.perf_counter()
    call(ticks)
    _sync()
    return (time.perf_counter() - t0) / ticks


def _vehicle_batch(B, device_vehicles):
    pool = [vars(scenarios.make_scenario(64, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0)))
            for k in range(POOL)]
    scenes = [pool[k % POOL] for k in range(B)]
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), 0.05, B=B)
    b.upload(scenes, device_vehicles=device_vehicles)
    return b, scenes


class _HostTraffic:
    """Form (c): every vehicle advanced on the host in the device's fp32 arithmetic (scenarios.advance_center_f32 /
    place_ring_f32, vectorised), then sent as rings with sfm_batch_set_dynamic_obstacles."""

    def __init__(self, b, scenes, dt):
        self.b = b
        self.item_off, self.off, ux, uy, cx, cy, yc, ys, vx, vy = pack_boxes(scenes)
        f64 = lambda a: a.astype(np.float64)
        self.u = (f64(ux), f64(uy))
        self.c = [f64(cx), f64(cy)]
        self.v = (f64(vx), f64(vy))
        self.dt = float(np.float32(dt))
        owner = np.repeat(np.arange(len(cx)), np.diff(self.off))   # vehicle of every ring point
        self.owner = owner
        self.rot = (f64(yc)[owner], f64(ys)[owner])

    def step(self):
        self.b.run(1)                                              # tick t sees the vehicles at c_t, as with (b)
        f32 = lambda a: a.astype(np.float32)
        self.c = [f32(self.dt * v + c).astype(np.float64) for c, v in zip(self.c, self.v)]
        (ux, uy), (cs, sn) = self.u, self.rot
        cx, cy = self.c[0][self.owner], self.c[1][self.owner]
        px = f32(cs * ux + f32(-sn * uy + cx).astype(np.float64))
        py = f32(sn * ux + f32(cs * uy + cy).astype(np.float64))
        arrs = [px, py, f32(self.c[0]), f32(self.c[1]), f32(self.v[0]), f32(self.v[1])]
        rc = self.b._lib.sfm_batch_set_dynamic_obstacles(self.b._b, iptr(self.item_off), iptr(self.off), *(fptr(a) for a in arrs))
        assert rc == 0, rc


def _time_vehicles(form, b, traffic, ticks):
    step = traffic.step if form == "c" else (lambda: b.run(1))
    call = (lambda k: b.run(k)) if form != "c" else (lambda k: [step() for _ in range(k)])
    call(3)
    _sync()
    t0 = time.perf_counter()
    call(ticks)
    _sync()
    return (time.perf_counter() - t0) / ticks


def _time_handles(B, n, geo, ticks):
    pool = _pool(n, geo)
    cfg = default_sfm_config(scenarios.ALL_FORCES if geo else PED)
    engs = []
    try:
        for k in range(B):
            sc = pool[k % POOL]
            e = SfmEngine(cfg, 0.05)
            engs.append(e)
            e.set_timing(False)                      # no HIP-event bracket per call: the handles' best case
            if geo:
                e.set_borders(sc["borders"], sc["border_centers"], sc["border_lengths"])
                e.set_static_obstacles(sc["static_obstacles"])
                e.set_dynamic_obstacles(sc["dynamic_obstacles"], sc["dynamic_vel"])
            e.upload_state(sc["loc"], sc["vel"], sc["waypoint"], sc["target_speed"], sc["radius"], None)
        for e in engs:
            e.run(1)
        _sync()
        t0 = time.perf_counter()
        for _ in range(ticks):
            for e in engs:
                e.run(1)
        _sync()
        dt = time.perf_counter() - t0
    finally:
        for e in engs:
            e.close()
    return dt / ticks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("batch", "handles", "trace", "streams", "plain", "trace-recorded", "vehicles",
                                       "rings", "trace-vehicles"), required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=50)
    args = ap.parse_args()
    if args.part == "batch":
        print("# batch: one launch per tick for the whole batch (SfmBatch.run)")
        print(f"{'forces':<10} {'B':>6} {'N_b':>5} {'us/tick':>10} {'scene-ticks/s':>14} {'ped-ticks/s':>12}")
        for geo in (False, True):
            for B in (64, 1024, 8192):
                for n in (20, 64, 256):
                    t = _time_batch(B, n, geo, args.ticks)
                    print(f"{'all five' if geo else 'ped+acc':<10} {B:>6} {n:>5} {t * 1e6:>10.1f} {B / t:>14.3e} {B * n / t:>12.3e}",
                          flush=True)
    elif args.part == "handles":
        print("# handles: B separate SfmEngine handles, run(1) each in a loop (HIP-event timing off), N_b = 64")
        print(f"{'forces':<10} {'B':>6} {'N_b':>5} {'us/tick':>10} {'scene-ticks/s':>14} {'batch us/tick':>14} {'batch speed-up':>15}")
        for geo in (False, True):
            for B in (64, 1024):
                th = _time_handles(B, 64, geo, max(3, args.ticks // 5))
                tb = _time_batch(B, 64, geo, args.ticks)
                print(f"{'all five' if geo else 'ped+acc':<10} {B:>6} {64:>5} {th * 1e6:>10.1f} {B / th:>14.3e} {tb * 1e6:>14.1f} "
                      f"{th / tb:>14.1f}x", flush=True)
    elif args.part in ("streams", "plain"):
        modes = ("plain", "redraw", "recorded", "stepwise") if args.part == "streams" else ("plain",)
        lib = "the SFM_LIB_PATH build" if os.environ.get("SFM_LIB_PATH") else "the in-tree build"
        print(f"# {args.part}: B scenes of 64, ped+acc, {args.ticks} ticks per call, modes alternated in {args.rounds} rounds; "
              f"library: {lib}")
        print(f"{'mode':<10} {'B':>6} {'N_b':>5} {'round':>5} {'us/tick':>10} {'scene-ticks/s':>14}")
        for B in (1024, 8192):
            b, sides = _streams_batch(B, 64)
            try:
                if "redraw" in modes:
                    b.set_waypoint_streams(np.arange(B), sides, 2.0)
                for r in range(args.rounds):
                    for mode in modes:
                        t = _time_mode(b, mode, args.ticks)
                        print(f"{mode:<10} {B:>6} {64:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
                assert all(np.isfinite(v).all() for _, v in b.state()[:POOL])
                if "redraw" in modes:
                    print(f"# B = {B}: {sum(int(d.sum()) for _, d in b.waypoints())} waypoint draws in all", flush=True)
            finally:
                b.close()
    elif args.part == "vehicles":
        B = 1024
        print(f"# vehicles: B = {B} scenes of 64, all five forces, 4 vehicles per scene; {args.ticks} ticks per call, forms alternated "
              f"in {args.rounds} rounds: (a) rings never moved, (b) device-side vehicles, (c) host twin + set_dynamic_obstacles per tick")
        print(f"{'form':<6} {'B':>6} {'N_b':>5} {'round':>5} {'us/tick':>10} {'scene-ticks/s':>14}")
        batches = {f: _vehicle_batch(B, f == "b") for f in "abc"}
        try:
            traffic = _HostTraffic(*batches["c"], 0.05)
            for r in range(args.rounds):
                for f in "abc":
                    t = _time_vehicles(f, batches[f][0], traffic, args.ticks)
                    print(f"{f:<6} {B:>6} {64:>5} {r:>5} {t * 1e6:>10.1f} {B / t:>14.3e}", flush=True)
            # (b) and (c) computed the same traffic: after the same number of ticks the vehicles agree bit for bit
            vb, vc = batches["b"][0].dynamic_obstacles(), batches["c"][0].dynamic_obstacles()
            same = all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for sb, sc in zip(vb, vc) for x, y in zip(sb, sc))
            print(f"# vehicles of (b) and (c) after {args.rounds * (args.ticks + 3)} ticks: {'bitwise equal' if same else 'DIFFER'}")
            assert same
            assert all(np.isfinite(v).all() for f in "abc" for _, v in batches[f][0].state()[:POOL])
        finally:
            for b, _ in batches.values():
                b.close()
    elif args.part == "rings":
        lib = "the SFM_LIB_PATH build" if os.environ.get("SFM_LIB_PATH") else "the in-tree build"
        b, _ = _vehicle_batch(1024, False)
        try:
            ta = min(_time_vehicles("a", b, None, args.ticks) for _ in range(args.rounds))
        finally:
            b.close()
        tg = min(_time_batch(1024, 64, True, args.ticks) for _ in range(args.rounds))
        print(f"rings  1024 x 64, {args.ticks} ticks, best of {args.rounds}, {lib}: form (a) {ta * 1e6:.1f} us/tick, "
              f"`batch` all five {tg * 1e6:.1f} us/tick", flush=True)
    elif args.part == "trace-vehicles":
        b, _ = _vehicle_batch(1024, True)
        try:
            b.run(3)
            _sync()
            t0 = time.perf_counter()
            b.run(args.ticks)
            _sync()
            t = (time.perf_counter() - t0) / args.ticks
        finally:
            b.close()
        print(f"# trace-vehicles: B = 1024, N_b = 64, all five forces, 4 device-side vehicles per scene: one set_dynamic_boxes, then "
              f"3 warm-up + {args.ticks} timed ticks = {args.ticks + 3} launches of sfm_batch_tick_kernel and 1 of "
              f"sfm_dynamic_boxes_kernel expected; {t * 1e6:.1f} us per tick (wall clock, under the tracer)")
    elif args.part == "trace-recorded":
        b, _ = _streams_batch(1024, 64)
        try:
            b.run(3)
            frames, idx, _ = b.run_recorded(args.ticks, stride=1)
            _sync()
        finally:
            b.close()
        print(f"# trace-recorded: B = 1024, N_b = 64, ped+acc: 3 plain warm-up ticks + run_recorded({args.ticks}, stride=1) -> "
              f"{len(idx)} frames of {frames[0].shape[1]} pedestrians per scene; expected: 3 launches of "
              f"sfm_batch_tick_kernel<.., false> and {args.ticks} of the recording sfm_batch_tick_kernel<.., true>")
    else:
        t = _time_batch(1024, 64, False, args.ticks)
        print(f"# trace: B = 1024, N_b = 64, ped+acc: {args.ticks} timed + 3 warm-up batch ticks = {args.ticks + 3} launches "
              f"of sfm_batch_tick_kernel expected; {t * 1e6:.1f} us per tick (wall clock, under the tracer)")


if __name__ == "__main__":
    main()
