"""Observed tracks on a batch (sfm_batch_set_observed, sfm_batch_run_observed, sfm_batch_score): B = 1024 scenes of 64, all five
forces, 4 moving device-side vehicles per scene, one scored row per scene and 63 replayed ones, every = 1, 50 frames.
  --part existing  `rounds` rounds of run(ticks) and `ticks` x restart_device() of a batch WITHOUT observed tracks -- run once per
                   library build (SFM_LIB_PATH names another build) and alternated by tools/batch_replay.sh: this build against its
                   parent
  --part replay    alternated in `rounds` rounds (us per tick or per call, medians at the end):
                   (ro) run_observed(0, ticks): one frame kernel and one tick per frame, nothing copied;
                   (t)  run(ticks) of the same batch, for scale: (ro) - (t) is what the frame kernels add;
                   (sc) score(), `ticks` calls;
                   (ss) scene_scores(): score() and the copy of B x 5 floats, `ticks` calls;
                   (old) what a caller had before: per tick set_commands (one copy of the commands) and run_recorded(1) (one tick
                        and the download of its frame), then the ADE of the scored rows in NumPy
  --part trace     `ticks` frames of run_observed and `ticks` x score() -- for rocprofv3 --kernel-trace: the duration of one
                   sfm_batch_replay_kernel and one sfm_batch_score_kernel launch beside one tick
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
from carla_social_force_model_amd.batch import SfmBatch  # noqa: E402
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


def _scenes(B):
    pool = [vars(scenarios.make_scenario(N_B, 7000 + k, n_borders=2, n_static=2, n_dynamic=4, border_len=(2.0, 2.0))) for k in range(POOL)]
    return [pool[k % POOL] for k in range(B)]


def _batch(B):
    b = SfmBatch(default_sfm_config(scenarios.ALL_FORCES), DT, B=B)
    b.upload(_scenes(B), device_vehicles=True)
    return b


def _tracks(scenes, F):
    """Every row walks on from where it stands with its uploaded velocity; row 0 of each scene is scored, the others replayed."""
    out = []
    for sc in scenes:
        loc, vel = np.asarray(sc["loc"], np.float64)[:, :2], np.asarray(sc["vel"], np.float64)[:, :2]
        out.append(np.stack([np.float32(loc + f * DT * vel) for f in range(F)]))
    roles = [np.r_[2, np.ones(N_B - 1)].astype(np.uint8)] * len(scenes)
    return out, roles


def part_existing(a):
    b = _batch(a.B)
    b.snapshot()
    import torch
    mask = torch.zeros(a.B, dtype=torch.uint8, device="cuda")
    mask[::8] = 1
    b.run(3)
    for r in range(a.rounds):
        t = _timed(lambda: b.run(a.ticks))
        print(f"{a.label:<8} {'run(%d), per tick' % a.ticks:<32} {r:>5} {1e6 * t / a.ticks:>10.2f}")
        t = _timed(lambda: [b.restart_device(mask) for _ in range(a.ticks)])
        print(f"{a.label:<8} {'restart_device, every 8th scene':<32} {r:>5} {1e6 * t / a.ticks:>10.2f}")
    b.close()


def part_replay(a):
    scenes = _scenes(a.B)
    tracks, roles = _tracks(scenes, a.ticks)
    b = _batch(a.B)
    b.set_observed(tracks, roles, 1)
    old = _batch(a.B)
    kinds = np.concatenate(roles) == 1
    old.set_steering(kinds.astype(np.uint8))
    so = old.scene_off
    flat = np.concatenate([t.reshape(a.ticks, -1, 2) for t in tracks], axis=1)            # (F, N_total, 2)
    cmds = np.zeros((a.ticks, flat.shape[1], 3))
    cmds[:-1, :, :2] = (flat[1:] - flat[:-1]) / DT
    scored = np.flatnonzero(np.concatenate(roles) == 2)

    def old_path():
        err = []
        for t in range(a.ticks):
            old.set_commands(cmds[t])
            frames, _, _ = old.run_recorded(1)
            now = np.concatenate([fr[0, :, :2] for fr in frames])
            err.append(np.linalg.norm(now[scored] - flat[t, scored], axis=1))
        return np.mean(err, axis=0)

    b.run_observed(0, 3)
    old_path()
    res = {k: [] for k in ("ro", "t", "sc", "ss", "old")}
    print("# (a) us per tick (ro, t, old) or per call (sc, ss), per round")
    print(f"{'what':<44} {'round':>5} {'us':>10}")
    names = {"ro": "run_observed(0, %d), per tick" % a.ticks, "t": "run(%d), per tick" % a.ticks, "sc": "score()",
             "ss": "scene_scores(): score() + copy of B x 5", "old": "set_commands + run_recorded(1) + NumPy, per tick"}
    for r in range(a.rounds):
        res["ro"].append(_timed(lambda: b.run_observed(0, a.ticks)))
        res["t"].append(_timed(lambda: b.run(a.ticks)))
        res["sc"].append(_timed(lambda: [b.score() for _ in range(a.ticks)]))
        res["ss"].append(_timed(lambda: [b.scene_scores() for _ in range(a.ticks)]))
        res["old"].append(_timed(old_path))
        for k in res:
            print(f"{names[k]:<44} {r:>5} {1e6 * res[k][-1] / a.ticks:>10.2f}")
    print("# medians")
    for k in res:
        print(f"{names[k]:<44} {'med':>5} {1e6 * statistics.median(res[k]) / a.ticks:>10.2f}")
    b.close()
    old.close()


def part_trace(a):
    scenes = _scenes(a.B)
    tracks, roles = _tracks(scenes, a.ticks)
    b = _batch(a.B)
    b.set_observed(tracks, roles, 1)
    b.run(3)
    b.run_observed(0, a.ticks)
    for _ in range(a.ticks):
        b.score()
    _sync()
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("existing", "replay", "trace"), required=True)
    ap.add_argument("--label", default="this")
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    {"existing": part_existing, "replay": part_replay, "trace": part_trace}[a.part](a)


if __name__ == "__main__":
    main()
