"""A calibration sweep against recorded motion with no host in the loop (Johansson et al. 2007).

    python examples/batch_calibration_sweep.py [--peds 24] [--frames 40] [--every 2] [--grid 9]

One recording, grid x grid candidates for the pedestrian force's (A, lambda), one scene of the batch per candidate
(carla_social_force_model_amd.batch, "Observed tracks").  The recording is made here by the model itself under "true" parameters, so
that the sweep has an answer: everybody walks freely, and the positions every ``every`` ticks are the tracks.  Then a few
pedestrians are scored (simulated by the model under the candidate's parameters and compared with their tracks) and everybody else
is replayed along the recording.
    set_observed(tracks, roles, every, v0)    once: the recording, the roles and the scored rows' first velocities go to the device
    run_observed(0, F)                        per frame one frame kernel and ``every`` ticks; the error sums stay on the device
    score()                                   one launch: per scene {rows, samples, sum_d, sum_d2, sum_final_d}
    argmin of sum_d / samples                 torch, on the device: the candidate with the smallest average displacement error
The only thing that crosses to the host is the index of the best candidate (and, for the printout, B x 5 floats).
Needs an MI355X; importing this file does not."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DT = 0.05
TRUE_A, TRUE_LAMBDA = 4.5, 2.0
FORCES = ("acceleration_force", "pedestrian_force")


def config(a, lam):
    from carla_social_force_model_amd.config import default_sfm_config
    cfg = default_sfm_config(FORCES)
    cfg["pedestrian_force"].update({"A": float(a), "lambda": float(lam)})
    return cfg


def record(scene, frames, every):
    """The recording: (frames, n, 2) positions and the first velocities, from one free run under the true parameters."""
    from carla_social_force_model_amd.batch import SfmBatch
    b = SfmBatch(config(TRUE_A, TRUE_LAMBDA), DT, B=1)
    try:
        b.upload([scene])
        out = []
        for _ in range(frames):
            loc, _ = b.state()[0]
            out.append(np.float32(loc[:, :2]))
            b.run(every)
        return np.stack(out)
    finally:
        b.close()


def candidates(grid):
    a = TRUE_A * np.linspace(0.5, 1.5, grid)
    lam = TRUE_LAMBDA * np.linspace(0.5, 1.5, grid)
    return [(x, y) for x in a for y in lam]


def main():
    import torch
    from carla_social_force_model_amd import replay, scenarios
    from carla_social_force_model_amd.batch import SfmBatch
    ap = argparse.ArgumentParser()
    ap.add_argument("--peds", type=int, default=24)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--every", type=int, default=2)
    ap.add_argument("--grid", type=int, default=9)
    a = ap.parse_args()

    scene = vars(scenarios.make_scenario(a.peds, 4242, density=0.6))
    tracks = record(scene, a.frames, a.every)
    scored = np.arange(0, a.peds, 6)
    roles = np.ones(a.peds, np.uint8)
    roles[scored] = replay.ROLE_SCORED
    v0 = np.full((a.peds, 2), np.nan, np.float32)
    v0[scored] = np.float32(np.asarray(scene["vel"])[scored, :2])      # the scored rows start with the velocity they had

    cand = candidates(a.grid)
    B = len(cand)
    b = SfmBatch([config(x, y) for x, y in cand], DT)
    try:
        b.upload([scene] * B)
        b.set_stream(torch.cuda.current_stream().cuda_stream)
        b.set_observed([tracks] * B, [roles] * B, a.every, [v0] * B)
        b.run_observed(0, a.frames)
        b.score()
        s = b.scene_score_tensor()
        ade = s[:, replay.SC_SUM_D] / s[:, replay.SC_SAMPLES]
        best = int(torch.argmin(ade).item())
        table = b.scene_scores()
    finally:
        b.close()
    ade, rmse, fde = replay.metrics(table)
    print(f"{B} candidates over one recording of {a.frames} frames, {len(scored)} scored rows of {a.peds}")
    for k in np.argsort(ade)[:5]:
        print(f"  A = {cand[k][0]:5.2f}  lambda = {cand[k][1]:4.2f}   ADE {ade[k]:.5f} m  RMSE {rmse[k]:.5f} m  FDE {fde[k]:.5f} m")
    print(f"best: A = {cand[best][0]:.2f}, lambda = {cand[best][1]:.2f}  (truth: A = {TRUE_A}, lambda = {TRUE_LAMBDA})")


if __name__ == "__main__":
    main()
