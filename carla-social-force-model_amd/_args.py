"""Per-scene arguments of a batch, as ``batch`` and ``scan`` take them: a scalar (broadcast to every scene) or B values.  One check of
shape, dtype kind and broadcast, one of a length in metres on top of it, and the check of the ``frame`` argument.  Pure NumPy."""
from __future__ import annotations

import numpy as np

MAX_METRES = 1.0e6               # SFM_BATCH_MAX_SENSE_RANGE: the bound of every sense range, scan range and radius
FRAME_WORLD, FRAME_HEADING = 0, 1


def per_scene(v, name, B, kinds="iuf", shape_first=False):
    """``v`` -> a (B,) view of it, broadcast from a scalar or a single value.  ``kinds``: the dtype kinds it may have ("iu" reads
    "integers" in the refusal, anything else "numbers").  ``shape_first``: a value wrong in both ways is refused for its shape."""
    a = np.asarray(v)
    bad_shape = a.ndim > 1 or (a.ndim == 1 and a.shape[0] not in (1, B))
    if a.dtype.kind not in kinds and not (shape_first and bad_shape):
        raise ValueError(f"{name} must be {'integers' if kinds == 'iu' else 'numbers'}, got {a.dtype}")
    if bad_shape:
        raise ValueError(f"{name}: expected a scalar or {B} values, got shape {a.shape}")
    return np.broadcast_to(a.reshape(-1), (B,))


def per_scene_metres(v, name, B, strict):
    """``per_scene`` for a length in metres -> float32 [B]: finite, > 0 (``strict``) or >= 0, and <= 1e6 in float32, which is what
    the library would refuse."""
    with np.errstate(over="ignore"):
        r = np.ascontiguousarray(per_scene(v, name, B), dtype=np.float32)
    if not (np.isfinite(r).all() and ((r > 0).all() if strict else (r >= 0).all()) and (r <= np.float32(MAX_METRES)).all()):
        raise ValueError(f"{name} must be finite, {'> 0' if strict else '>= 0'} and <= {MAX_METRES:g} metres")
    return r


def check_frame(frame):
    """The ``frame`` of observations and scans -> int 0 (world axes) or 1 (the row's heading frame).  Raises ValueError."""
    if isinstance(frame, (bool, np.bool_)) or not isinstance(frame, (int, np.integer)) or int(frame) not in (FRAME_WORLD, FRAME_HEADING):
        raise ValueError(f"frame must be 0 (world axes) or 1 (the row's heading frame), got {frame!r}")
    return int(frame)
