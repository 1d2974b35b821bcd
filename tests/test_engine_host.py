"""CPU tests of SfmEngine's host side against a fake library: which buffer addresses the step calls hand to sfm_step_packed /
sfm_step_records when the caller changes arrays between calls, and which vehicle count dynamic_obstacles() sizes its buffers for
after the vehicles change.  No GPU, no libsfm_hip: ``_lib`` is replaced by a recorder."""
import ctypes as C

import numpy as np
import pytest

from carla_social_force_model_amd.engine import SfmEngine
from carla_social_force_model_amd.host_state import PED_STATE_DTYPE


def _floats(addr, n):
    return np.ctypeslib.as_array((C.c_float * n).from_address(addr)).copy() if n else np.zeros(0, np.float32)


class _FakeLib:
    """Records the arguments of every step call; keeps the vehicles it is given, as the library does, and hands them back."""

    def __init__(self):
        self.calls = []
        self.dyn = (np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32))

    def sfm_step_packed(self, h, n, p_rows, p_zvz, flags, p_out):
        self.calls.append({"n": n, "rows": p_rows, "zvz": p_zvz, "out": p_out})
        return 0

    def sfm_step_records(self, h, n, p_rec, stride, p_off, p_border, tol, flags, p_out, p_flag):
        off = np.ctypeslib.as_array((C.c_int32 * 5).from_address(p_off)).copy()
        self.calls.append({"n": n, "rec": p_rec, "stride": stride, "off": off, "out": p_out})
        return 0

    def sfm_set_dynamic_obstacles(self, h, M, off, px, py, cx, cy, vx, vy):
        P = int(np.ctypeslib.as_array((C.c_int32 * (M + 1)).from_address(off))[M]) if M else 0
        self.dyn = (_floats(cx, M), _floats(cy, M), _floats(px, P), _floats(py, P))
        return 0

    def sfm_set_dynamic_obstacles_packed(self, h, M, off, pts, cv):
        P = int(np.ctypeslib.as_array((C.c_int32 * (M + 1)).from_address(off))[M]) if M else 0
        p, c = _floats(pts, 2 * P).reshape(P, 2), _floats(cv, 4 * M).reshape(M, 4)
        self.dyn = (c[:, 0].copy(), c[:, 1].copy(), p[:, 0].copy(), p[:, 1].copy())
        return 0

    def sfm_set_dynamic_boxes(self, h, M, off, ux, uy, cx, cy, yc, ys, vx, vy):
        P = int(np.ctypeslib.as_array((C.c_int32 * (M + 1)).from_address(off))[M]) if M else 0
        self.dyn = (_floats(cx, M), _floats(cy, M), _floats(ux, P), _floats(uy, P))     # (unrotated: only the sizes matter here)
        return 0

    def sfm_download_dynamic_obstacles(self, h, cx, cy, px, py):
        for addr, a in zip((cx, cy, px, py), self.dyn):
            if len(a):
                C.memmove(addr, a.ctypes.data, a.nbytes)
        return 0


def _engine():
    eng = object.__new__(SfmEngine)
    eng._lib, eng._h = _FakeLib(), C.c_void_p(1)
    eng.n, eng.shard, eng.planar, eng._z0 = 0, (0, 0), True, 0.0
    eng._dyn_shape = (0, 0, np.zeros(1, np.int32))
    return eng


def _rows(n, seed):
    return np.random.default_rng(seed).uniform(-5, 5, (n, 9)).astype(np.float32)


def test_step_packed_passes_the_arrays_of_this_call():
    eng = _engine()
    kept = []
    for k, n in enumerate((10, 10, 7, 30)):                  # fresh owning arrays every call
        rows, out = _rows(n, k), np.full((n, 3), np.nan, np.float32)
        kept += [rows, out]
        eng.step_packed(rows, None, out)
        call = eng._lib.calls[-1]
        assert (call["n"], call["rows"], call["out"], call["zvz"]) == (n, rows.ctypes.data, out.ctypes.data, None)
    base_rows, base_out = _rows(64, 9), np.zeros((64, 3), np.float32)
    for lo, hi in ((0, 20), (0, 40), (8, 20), (30, 64), (0, 5)):        # prefixes and non-prefix slices of one kept base
        zvz = np.zeros((hi - lo, 2), np.float32)
        eng.step_packed(base_rows[lo:hi], zvz, base_out[lo:hi])
        call = eng._lib.calls[-1]
        assert call["rows"] == base_rows.ctypes.data + lo * 36 and call["out"] == base_out.ctypes.data + lo * 12
        assert call["zvz"] == zvz.ctypes.data and call["n"] == hi - lo and not eng.planar


def test_step_packed_rejects_buffers_of_the_wrong_shape_or_layout():
    eng = _engine()
    rows = _rows(8, 1)
    for out in (np.zeros((7, 3), np.float32), np.zeros((8, 4), np.float32)[:, :3]):
        with pytest.raises((ValueError, AssertionError)):
            eng.step_packed(rows, None, out)
    with pytest.raises((ValueError, AssertionError)):
        eng.step_packed(rows, np.zeros((7, 2), np.float32), np.zeros((8, 3), np.float32))
    with pytest.raises((ValueError, AssertionError)):
        eng.step_packed(rows.astype(np.float64), None, np.zeros((8, 3), np.float32))
    assert eng._lib.calls == []


def test_step_records_passes_the_arrays_of_this_call():
    eng = _engine()
    kept = []
    for k, n in enumerate((12, 12, 5)):                       # fresh owning records and v_out every call
        rec, out = np.zeros(n + 3, dtype=PED_STATE_DTYPE), np.full((n, 3), np.nan, np.float32)
        kept += [rec, out]
        eng.step_records(rec, n, None, out)
        call = eng._lib.calls[-1]
        assert (call["n"], call["rec"], call["stride"], call["out"]) == (n, rec.ctypes.data, rec.dtype.itemsize, out.ctypes.data)
    rec = kept[0]
    for n in (12, 12, 9):                                     # the same records, a fresh owning v_out every call
        out = np.full((n, 3), np.nan, np.float32)
        kept.append(out)
        eng.step_records(rec, n, None, out)
        assert (eng._lib.calls[-1]["rec"], eng._lib.calls[-1]["out"]) == (rec.ctypes.data, out.ctypes.data)
    base, out = np.zeros(40, dtype=PED_STATE_DTYPE), np.zeros((40, 3), np.float32)
    for sl in (slice(0, 20), slice(10, 30), slice(0, 40, 2), slice(3, 40, 3)):     # views of one base: offset and stride change
        v = base[sl]
        n = len(v)
        eng.step_records(v, n, None, out[:n])
        call = eng._lib.calls[-1]
        assert call["rec"] == base.ctypes.data + sl.start * base.dtype.itemsize
        assert call["stride"] == (sl.step or 1) * base.dtype.itemsize and call["out"] == out.ctypes.data


def test_step_records_reads_the_field_offsets_of_each_layout():
    eng = _engine()
    plain = np.zeros(6, dtype=PED_STATE_DTYPE)
    wide = np.zeros(6, dtype=[("pad", "u1", (13,))] + PED_STATE_DTYPE + [("tail", "f4")])
    names = ("loc", "vel", "next_waypoint", "radius", "target_speed")
    for rec in (plain, wide, plain):
        eng.step_records(rec, 6, None, np.zeros((6, 3), np.float32))
        call = eng._lib.calls[-1]
        assert list(call["off"]) == [rec.dtype.fields[k][1] for k in names] and call["stride"] == rec.dtype.itemsize
    assert eng._lib.calls[1]["stride"] == plain.dtype.itemsize + 17
    with pytest.raises(ValueError):
        eng.step_records(plain, 7, None, np.zeros((7, 3), np.float32))            # more rows than records
    bad = np.zeros(4, dtype=[(k, "f4" if k == "radius" else t, *s) for k, t, *s in PED_STATE_DTYPE])
    with pytest.raises(TypeError):
        eng.step_records(bad, 4, None, np.zeros((4, 3), np.float32))


def _rings(M, seed, base_len=5):
    rng = np.random.default_rng(seed)
    return ([rng.uniform(0, 50, 2) for _ in range(M)], [rng.uniform(0, 50, (base_len + k, 2)) for k in range(M)])


def _assert_vehicles(eng, ctr, rings):
    M, P = len(rings), sum(len(r) for r in rings)
    assert eng._dyn_shape[:2] == (M, P)               # (checked first: dynamic_obstacles() sizes its buffers from it)
    got = eng.dynamic_obstacles()
    assert len(got) == M
    for (c_g, r_g), c, r in zip(got, ctr, rings):
        assert np.array_equal(c_g, np.float32(c).astype(np.float64)) and np.array_equal(r_g, np.float32(r).astype(np.float64))


def test_dynamic_obstacles_follow_every_change_of_the_vehicles():
    eng = _engine()
    assert eng.dynamic_obstacles() == []
    c10 = [np.array([1.0 * k, 2.0]) for k in range(10)]
    eng.set_dynamic_boxes(c10, np.zeros(10), np.full((10, 2), [2.4, 1.0]), np.zeros((10, 2)))
    assert eng._dyn_shape[0] == 10
    c3, r3 = _rings(3, 1)
    eng.set_dynamic_obstacles(list(zip(c3, r3)), np.ones((3, 2)))                 # M 10 -> 3
    _assert_vehicles(eng, c3, r3)
    c8, r8 = _rings(8, 2, 9)
    eng.set_dynamic_obstacles(list(zip(c8, r8)))                                  # 3 -> 8, larger rings
    _assert_vehicles(eng, c8, r8)
    c3b, r3b = _rings(3, 3)
    eng.set_dynamic_vehicles(c3b, r3b, np.zeros((3, 2)))                          # 8 -> 3 through the packed report
    _assert_vehicles(eng, c3b, r3b)
    eng.set_dynamic_obstacles(list(zip(c8, r8)))                                  # 3 -> 8 ...
    _assert_vehicles(eng, c8, r8)
    c3c, r3c = _rings(3, 4)                                                       # ... and back with the ring sizes of the kept report
    eng.set_dynamic_vehicles(c3c, r3c, None)
    _assert_vehicles(eng, c3c, r3c)
    eng.set_dynamic_vehicles([], [], None)                                        # 0
    assert eng._dyn_shape[:2] == (0, 0) and eng.dynamic_obstacles() == []
    eng.set_dynamic_obstacles(list(zip(c8, r8)))
    eng.set_dynamic_obstacles(None)
    assert eng._dyn_shape[:2] == (0, 0) and eng.dynamic_obstacles() == []
