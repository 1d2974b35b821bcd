"""The host twins of the batch's observed tracks (sfm_batch_set_observed / sfm_batch_run_observed / sfm_batch_score; the rules:
include/sfm_hip.h), and a packer that turns a recording into a scene.

The calibration protocol of Johansson et al. 2007: a few pedestrians are simulated by the model (role 2, *scored*), everybody else
replays the recorded motion (role 1, *replayed*), and the simulated ones are scored by their displacement from their own tracks.

``replay_frame`` is the NumPy twin of the frame kernel and ``score_scene`` that of the per-scene reduction, both bit for bit: every
value of the rules is one correctly rounded fp32 operation or an ``fmaf`` (``scan._fma32`` is an exact one), and the sums are
formed in the kernel's own order.  ``scene_from_tracks`` builds a scene dict, roles and initial velocities from a ``(F, n, 2)``
array with NaNs.

Pure NumPy, no GPU and no library needed.
"""
from __future__ import annotations

import numpy as np

from ._args import MAX_METRES
from .scan import _fma32

ROLE_NONE, ROLE_REPLAYED, ROLE_SCORED = 0, 1, 2      # SFM_ROLE_*
MAX_OBSERVED_FRAMES = 16384                          # SFM_BATCH_MAX_OBSERVED_FRAMES
SCENE_SCORE_WIDTH = 5                                # SFM_BATCH_SCENE_SCORE_WIDTH
SC_ROWS, SC_SAMPLES, SC_SUM_D, SC_SUM_D2, SC_SUM_FINAL_D = range(5)

_BLOCK, _WAVE = 256, 64
_FAR_AWAY, _FAR_STEP = float(np.float32(3.0e15)), float(np.float32(1.0e12))


def park_positions(n):
    """Where rows 0 .. n-1 of a scene are parked, (n, 2) float32: park_position of the index inside the scene, as the device
    computes it -- FAR_AWAY + FAR_STEP * (i + 1) by one fused multiply-add (the float64 expression is exact, so it is rounded
    once), and y = -FAR_AWAY."""
    i = np.arange(n, dtype=np.float64)
    return np.stack([(_FAR_AWAY + _FAR_STEP * (i + 1)).astype(np.float32), np.full(n, -_FAR_AWAY, np.float32)], axis=1)


def frame_rate(every, step_length):
    """inv_h = float32(1 / (every * step_length)) with step_length as the fp32 value the library holds, formed in float64 and
    rounded once.  Raises ValueError where the library refuses: ``every`` < 1, or a product (or reciprocal) that is not finite
    and positive in fp32."""
    if isinstance(every, (bool, np.bool_)) or not isinstance(every, (int, np.integer)) or int(every) < 1:
        raise ValueError(f"every must be an integer >= 1 tick between two observed frames, got {every!r}")
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        h = float(int(every)) * float(np.float32(step_length))
        hf = np.float32(h)
        inv = np.float32(1.0 / h) if h != 0 else np.float32(np.inf)
    if not (np.isfinite(hf) and hf > 0 and np.isfinite(inv) and inv > 0):
        raise ValueError(f"every * step_length must be finite and positive in fp32 (every {every}, step_length {step_length})")
    return inv


def check_tracks(obs, n=None):
    """One scene's track frames -> (F, n, 2) float32.  NaN in BOTH components: the row is not seen in the frame; every other value
    finite and within 1e6 metres.  Raises ValueError on what the library refuses."""
    a = np.asarray(obs, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 2:
        raise ValueError(f"tracks must be a (F, n, 2) array, got shape {a.shape}")
    if n is not None and a.shape[1] != n:
        raise ValueError(f"tracks hold {a.shape[1]} rows, the scene {n}")
    if a.shape[0] > MAX_OBSERVED_FRAMES:
        raise ValueError(f"tracks hold {a.shape[0]} frames, more than {MAX_OBSERVED_FRAMES}")
    with np.errstate(over="ignore", invalid="ignore"):
        a32 = a.astype(np.float32)
    nx, ny = np.isnan(a32[..., 0]), np.isnan(a32[..., 1])
    if (nx != ny).any():
        raise ValueError("an observed position must be NaN in both components (not seen) or in none")
    ok = nx | ((np.abs(a32[..., 0]) <= np.float32(MAX_METRES)) & (np.abs(a32[..., 1]) <= np.float32(MAX_METRES)))
    if not ok.all():
        raise ValueError(f"an observed position must be finite and within {MAX_METRES:g} metres")
    return np.ascontiguousarray(a32)


def spans(obs):
    """(f0, f1) int32 (n,) each: the first and last frame a row is observed in; f0 = 1, f1 = 0 (empty) for a row never seen."""
    obs = np.asarray(obs, dtype=np.float32)
    F, n = obs.shape[0], obs.shape[1]
    seen = ~np.isnan(obs[..., 0]) if F else np.zeros((0, n), bool)
    any_ = seen.any(axis=0) if F else np.zeros(n, bool)
    f0 = np.where(any_, seen.argmax(axis=0) if F else 0, 1).astype(np.int32)
    f1 = np.where(any_, F - 1 - seen[::-1].argmax(axis=0) if F else 0, 0).astype(np.int32)
    return f0, f1


def new_scene(state):
    """The three buffers the frame kernel writes, for one scene of n rows: ``state`` (n, 4) float32 {x, y, vx, vy} as given,
    ``commands`` (n, 4) zeros, ``scores`` (n, 4) zeros."""
    st = np.array(state, dtype=np.float32).reshape(-1, 4)
    return {"state": st, "commands": np.zeros_like(st), "scores": np.zeros_like(st)}


def replay_frame(scene, obs, roles, v0, f, inv_h):
    """The frame kernel's twin for one scene, bit for bit.  ``scene``: a dict of ``state`` (n, 4) float32 {x, y, vx, vy},
    ``commands`` (n, 4) float32 {ux, uy, uz, kind} and ``scores`` (n, 4) float32 {samples, sum_d, sum_d2, last_d2} as they are before
    the launch; ``obs`` (F, n, 2) float32 with NaN where a row is not seen; ``roles`` (n,) 0 / 1 / 2; ``v0`` (n, 2) float32 with NaN
    for "take it from the track", or None; ``f`` the frame; ``inv_h`` the scene's ``frame_rate``.  Returns a new dict of the same
    three arrays as they are after it; rows of role 0 are copied through."""
    st = np.array(scene["state"], dtype=np.float32).reshape(-1, 4)
    cmd = np.array(scene["commands"], dtype=np.float32).reshape(-1, 4)
    sc = np.array(scene["scores"], dtype=np.float32).reshape(-1, 4)
    n = st.shape[0]
    obs = np.asarray(obs, dtype=np.float32)
    obs = obs.reshape(obs.shape[0] if obs.ndim == 3 else -1, n, 2)     # (a scene without rows still has its frames)
    F, f = obs.shape[0], int(f)
    roles = np.asarray(roles).astype(np.int64).reshape(n)
    v0 = np.full((n, 2), np.nan, np.float32) if v0 is None else np.asarray(v0, dtype=np.float32).reshape(n, 2)
    inv_h = np.float32(inv_h)
    nan2 = np.full((n, 2), np.nan, np.float32)
    at = lambda g: obs[g] if 0 <= g < F else nan2
    o, o1, om = at(f), at(f + 1), at(f - 1)
    seen, seen1, seenm = (~np.isnan(a[:, 0]) for a in (o, o1, om))
    f0, f1 = spans(obs)
    in_span = (f0 <= f1) & (f >= f0) & (f <= f1)
    rep, scd = roles == ROLE_REPLAYED, roles == ROLE_SCORED
    given = ~np.isnan(v0[:, 0])

    parked = (rep & ~seen) | (scd & ~in_span)
    st[parked, :2] = park_positions(n)[parked]
    st[parked, 2:] = 0
    cmd[parked] = np.float32([0, 0, 0, 1])

    with np.errstate(over="ignore", invalid="ignore"):
        fwd = ((o1 - o).astype(np.float32) * inv_h).astype(np.float32)
        bwd = ((o - om).astype(np.float32) * inv_h).astype(np.float32)
    zero = np.zeros((n, 2), np.float32)
    # role 1, observed at f: forward difference, else backward, else v0, else 0
    v1 = np.where(seen1[:, None], fwd, np.where(seenm[:, None], bwd, np.where(given[:, None], v0, zero)))
    # role 2 at its first frame: v0, else the forward difference, else 0
    v2 = np.where(given[:, None], v0, np.where(seen1[:, None], fwd, zero))
    place1 = rep & seen
    place2 = scd & in_span & (f == f0)
    for pick, v, kind in ((place1, v1, 1.0), (place2, v2, 0.0)):
        st[pick, :2] = o[pick]
        st[pick, 2:] = v[pick]
        cmd[pick] = 0
        if kind:
            cmd[pick, :2] = v[pick]
            cmd[pick, 3] = kind

    walk = scd & in_span & (f != f0)                                   # the model moves it: compare it with its track
    cmd[walk] = 0
    hit = walk & seen
    with np.errstate(over="ignore", invalid="ignore"):
        dx = (st[:, 0] - o[:, 0]).astype(np.float32)
        dy = (st[:, 1] - o[:, 1]).astype(np.float32)
        d2 = _fma32(dx, dx, (dy * dy).astype(np.float32))
        d = np.sqrt(d2, dtype=np.float32)
        new = np.stack([sc[:, 0] + np.float32(1), sc[:, 1] + d, sc[:, 2] + d2, d2], axis=1).astype(np.float32)
    sc[hit] = new[hit]
    return {"state": st, "commands": cmd, "scores": sc}


def score_scene(row_scores):
    """The per-scene reduction's twin, bit for bit: ``row_scores`` (n, 4) float32 {samples, sum_d, sum_d2, last_d2} ->
    (5,) float32 {rows, samples, sum_d, sum_d2, sum_final_d} over the rows with samples > 0, summed in the kernel's order: lane t of
    256 adds its rows t, t + 256, ... ascending from +0; an xor-shuffle tree of widths 32 .. 1 inside each wave of 64; then
    waves 0 .. 3 in ascending order."""
    q = np.asarray(row_scores, dtype=np.float32).reshape(-1, 4)
    n = q.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        take = q[:, 0] > 0
        terms = np.stack([np.ones(n, np.float32), q[:, 0], q[:, 1], q[:, 2], np.sqrt(q[:, 3], dtype=np.float32)], axis=1)
        lanes = np.zeros((_BLOCK, SCENE_SCORE_WIDTH), np.float32)
        for lo in range(0, n, _BLOCK):                                 # round r: lane t adds row t + 256 r
            m = min(_BLOCK, n - lo)
            t = np.flatnonzero(take[lo:lo + m])
            lanes[t] = lanes[t] + terms[lo + t]
        lane = np.arange(_BLOCK)
        s = _WAVE // 2
        while s >= 1:
            lanes = lanes + lanes[lane ^ s]
            s //= 2
        out = lanes[0].copy()
        for w in range(1, _BLOCK // _WAVE):
            out = out + lanes[w * _WAVE]
    return out.astype(np.float32)


def metrics(scene_scores):
    """{rows, samples, sum_d, sum_d2, sum_final_d} (..., 5) -> (ADE, RMSE, FDE) float64 (...,): sum_d / samples,
    sqrt(sum_d2 / samples), sum_final_d / rows; NaN where nothing was scored."""
    s = np.asarray(scene_scores, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s[..., SC_SUM_D] / s[..., SC_SAMPLES], np.sqrt(s[..., SC_SUM_D2] / s[..., SC_SAMPLES]), s[..., SC_SUM_FINAL_D] / s[..., SC_ROWS]


def scene_from_tracks(tracks, step_length, every, scored):
    """A recording -> what ``SfmBatch.upload`` and ``SfmBatch.set_observed`` take for one scene.  ``tracks`` (F, n, 2) with NaN
    where a pedestrian is not seen; ``step_length`` the scene's tick length and ``every`` the ticks between two frames (a frame
    lasts every * step_length seconds); ``scored``: the rows the model simulates (indices or a bool mask) -- everybody else who is
    ever seen is replayed, and a row that is never seen gets role 0.

    Returns (scene, roles, v0): ``scene`` a scene dict -- loc the first observed position (a row never seen: the origin), vel zeros
    (the frame kernel sets them), waypoint the LAST observed position, target_speed the mean observed speed (the path length between
    consecutive observed frames over the time between them; 0 with fewer than two) --, ``roles`` (n,) uint8, ``v0`` (n, 2) float32
    all NaN ("take it from the track")."""
    obs = check_tracks(tracks).astype(np.float64)
    F, n = obs.shape[0], obs.shape[1]
    h = float(int(every)) * float(step_length)
    frame_rate(every, step_length)
    f0, f1 = spans(obs.astype(np.float32))
    ever = f0 <= f1
    idx = np.arange(n)
    first = np.where(ever[:, None], obs[np.where(ever, f0, 0), idx] if F else 0.0, 0.0)
    last = np.where(ever[:, None], obs[np.where(ever, f1, 0), idx] if F else 0.0, 0.0)
    speed = np.zeros(n)
    for i in np.flatnonzero(ever):
        fr = np.flatnonzero(~np.isnan(obs[:, i, 0]))
        if len(fr) >= 2:
            speed[i] = np.linalg.norm(np.diff(obs[fr, i], axis=0), axis=1).sum() / ((fr[-1] - fr[0]) * h)
    pick = np.zeros(n, bool)
    pick[np.asarray(scored, dtype=bool) if np.asarray(scored).dtype == bool else np.asarray(scored, dtype=np.int64)] = True
    roles = np.where(ever, np.where(pick, ROLE_SCORED, ROLE_REPLAYED), ROLE_NONE).astype(np.uint8)
    z = np.zeros((n, 1))
    scene = {"loc": np.hstack([first, z]), "vel": np.zeros((n, 3)), "waypoint": np.hstack([last, z]), "target_speed": speed}
    return scene, roles, np.full((n, 2), np.nan, np.float32)


def pack_observed(tracks, roles, scene_off, v0=None):
    """Per-scene tracks and roles -> the arguments of sfm_batch_set_observed: (obs_off int64 [B+1], frames int32 [B], obs float32
    [total, 2], roles uint8 [N_total], v0 float32 [N_total, 2] or None).  ``tracks``: a list of B arrays (F_b, n_b, 2); ``roles``:
    a list of B arrays (n_b,) or one array over the concatenated rows; ``v0`` likewise with (n_b, 2), None entries (or None
    altogether) meaning NaN.  Pure NumPy; raises ValueError on a shape that does not fit and on every value the library refuses."""
    so = np.asarray(scene_off, dtype=np.int64)
    B, n = len(so) - 1, int(so[-1])
    tracks = list(tracks)
    if len(tracks) != B:
        raise ValueError(f"{len(tracks)} tracks for {B} scenes")
    obs = [check_tracks(t, int(so[b + 1] - so[b])) for b, t in enumerate(tracks)]
    frames = np.array([o.shape[0] for o in obs], dtype=np.int32)
    off = np.zeros(B + 1, np.int64)
    np.cumsum([o.shape[0] * o.shape[1] for o in obs], out=off[1:])
    flat = np.concatenate([o.reshape(-1, 2) for o in obs], axis=0) if B else np.zeros((0, 2), np.float32)

    def rows(v, width, name, fill):
        if isinstance(v, (list, tuple)) and len(v) == B and all(e is None or np.ndim(e) >= 1 for e in v):   # one entry per scene
            parts = []
            for b, e in enumerate(v):
                nb = int(so[b + 1] - so[b])
                a = np.full((nb, width) if width else nb, fill) if e is None else np.asarray(e)
                if a.shape != ((nb, width) if width else (nb,)):
                    raise ValueError(f"scene {b}: {name} has shape {a.shape}, expected {(nb, width) if width else (nb,)}")
                parts.append(a)
            return np.concatenate(parts, axis=0) if parts else np.zeros((0, width) if width else 0)
        a = np.asarray(v)
        if a.shape != ((n, width) if width else (n,)):
            raise ValueError(f"{name} has shape {a.shape}, expected {(n, width) if width else (n,)} over the concatenated rows")
        return a

    r = rows(roles, 0, "roles", 0)
    if r.size and not (np.all(r == np.round(r)) and r.min() >= 0 and r.max() <= ROLE_SCORED):
        raise ValueError("roles must be 0 (not part of the data), 1 (replayed) or 2 (scored)")
    r = np.ascontiguousarray(r, dtype=np.uint8)
    if v0 is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            v0 = np.ascontiguousarray(rows(v0, 2, "v0", np.nan), dtype=np.float32)
        if (np.isnan(v0[:, 0]) != np.isnan(v0[:, 1])).any() or np.isinf(v0).any():
            raise ValueError("v0 must be finite, or NaN in both components (take it from the track)")
    return off, frames, np.ascontiguousarray(flat, dtype=np.float32), r, v0
