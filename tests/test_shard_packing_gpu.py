"""The library's row packing against tests/_shards.pack_order on the GPU: the host packing of sfm_upload_state and the device re-pack
of sfm_resort (four rocPRIM radix sorts with a partition) must give the same permutation for the same state (DESIGN.md section 6;
every rank re-packs alone and relies on it).  The row order is read from the packed() rows and mapped back to the caller's index
through each pedestrian's unique (x, y)."""
import numpy as np
import pytest

import _shards as S
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd.config import default_sfm_config
from carla_social_force_model_amd.stepper import HipShardEngine, balanced_bounds, equal_bounds

pytestmark = pytest.mark.gpu

LAYOUTS = [None, (1, 2), (2, 1), (2, 2), (2, 4), (4, 2), (8, 1), (4, 4)]


def _crowd(kind, n):
    """make_scenario's crowd with its positions replaced: distinct (x, y) pairs in every kind"""
    sc = scenarios.make_scenario(n, 900 + n)
    rng = np.random.default_rng(n)
    x = rng.choice(10 ** 6, n, replace=False) * (150.0 / 10 ** 6)
    y = rng.choice(10 ** 6, n, replace=False) * (150.0 / 10 ** 6)
    if kind == "repeated_x":                     # 40 x values shared by many, y distinct; both signed zeros among them
        x = np.floor(x / 150.0 * 40.0) - 20.0
        x[x == 0.0] = np.where(np.arange(int((x == 0.0).sum())) % 2 == 0, 0.0, -0.0)
    elif kind == "elongated":                    # 1500 m by 1.5 m: the aspect clamp (64) is hit
        x = x * 10.0
        y = y / 100.0
    sc.loc[:, 0] = np.float32(x)
    sc.loc[:, 1] = np.float32(y)
    return sc


def _bounds_sets(n, n_pad, layout):
    if layout is None:
        return [None]
    g = layout[0] * layout[1]
    eq = equal_bounds(n, n_pad, g)
    skew = balanced_bounds(eq, [float(1 + 3 * r) for r in range(g)], n)
    empty = list(eq)
    if g > 2:
        empty[2] = empty[1]                      # two equal interior bounds: block 1 is empty
    else:
        empty[1] = 0                             # (G = 2: block 0 is)
    return [None, eq, skew, empty]


@pytest.mark.parametrize("kind", ["random", "repeated_x", "elongated"])
@pytest.mark.parametrize("n", [2048, 2049, 4352, 9000])
def test_upload_packs_like_pack_order(kind, n):
    sc = _crowd(kind, n)
    if kind == "repeated_x":
        assert (np.signbit(sc.loc[:, 0]) & (sc.loc[:, 0] == 0.0)).any() and (~np.signbit(sc.loc[:, 0]) & (sc.loc[:, 0] == 0.0)).any()
    if kind == "elongated":
        assert S.crowd_aspect(sc.loc[:, 0], sc.loc[:, 1]) == 64.0
    e = HipShardEngine(default_sfm_config(("acceleration_force", "pedestrian_force")), S.DT)
    try:
        checked = 0
        for layout in LAYOUTS:
            n_pad = -(-n // 256) * 256
            for bounds in _bounds_sets(n, n_pad, layout):
                e.engine.set_partition(*(layout or (0, 0)), bounds)
                e.load(sc)
                assert e.n_pad == n_pad
                got = S.rows_order(S.packed_rows(e, n)[:, :2], sc.loc[:, :2])
                want = S.pack_order(sc.loc[:, 0], sc.loc[:, 1], n_pad, layout, bounds)
                assert np.array_equal(got, want), f"layout {layout}, bounds {bounds}: {int((got != want).sum())} rows differ"
                checked += 1
        assert checked == 1 + 7 * 4
    finally:
        e.close()


@pytest.mark.parametrize("layout", [(1, 2), (2, 2), (2, 4), (4, 2), (8, 1), (4, 4), None], ids=lambda l: "plain" if l is None else f"{l[0]}x{l[1]}")
@pytest.mark.parametrize("n,z_spread", [(4352, 0.0), (9000, 1.5)])
def test_device_repack_packs_like_pack_order_and_like_a_fresh_upload(layout, n, z_spread, monkeypatch):
    """A crowd moved a few ticks with the automatic re-pack off, then sfm_resort: the device order is pack_order of the current state
    (with the aspect of the uploaded crowd, which the handle keeps), and the re-packed rows -- {x, y, vx, vy}, {z, vz}, waypoints,
    target speeds, radii -- equal a fresh upload of that state to a second handle with the same partition, bit for bit."""
    monkeypatch.setenv("SFM_RESORT_EVERY", "0")
    cfg = default_sfm_config(("acceleration_force", "pedestrian_force"))
    sc = scenarios.make_scenario(n, 300 + n, z_spread=z_spread)
    n_pad = -(-n // 256) * 256
    g = 1 if layout is None else layout[0] * layout[1]
    bounds = balanced_bounds(equal_bounds(n, n_pad, g), [float(2 + r % 3) for r in range(g)], n) if g > 1 else None
    moved, fresh = HipShardEngine(cfg, S.DT), HipShardEngine(cfg, S.DT)
    try:
        moved.engine.set_partition(*(layout or (0, 0)))
        moved.load(sc)
        moved.engine.set_partition(*(layout or (0, 0)), bounds)
        aspect = S.crowd_aspect(sc.loc[:, 0], sc.loc[:, 1])
        moved.run(6, redraw=False)
        moved.synchronize()
        loc, vel, wp = moved.engine.state()
        before = S.rows_order(S.packed_rows(moved, n)[:, :2], loc[:, :2])
        assert not np.array_equal(before, S.pack_order(loc[:, 0], loc[:, 1], n_pad, layout, bounds, aspect=aspect))   # stale
        moved.resort()
        moved.synchronize()
        got = S.rows_order(S.packed_rows(moved, n)[:, :2], loc[:, :2])
        want = S.pack_order(loc[:, 0], loc[:, 1], n_pad, layout, bounds, aspect=aspect)
        assert np.array_equal(got, want), f"{int((got != want).sum())} rows differ from pack_order"
        # a fresh upload takes the aspect of the moved crowd: the same strips here (checked), hence the same rows
        assert np.array_equal(want, S.pack_order(loc[:, 0], loc[:, 1], n_pad, layout, bounds))
        st = scenarios.make_scenario(n, 300 + n, z_spread=z_spread)
        st.loc, st.vel = loc, vel
        st.waypoint = np.concatenate([wp, np.zeros((n, 1))], axis=1)
        fresh.engine.set_partition(*(layout or (0, 0)), bounds)
        fresh.load(st)
        fresh.synchronize()
        for (a, w), (b, _) in zip(moved.packed(), fresh.packed()):
            assert np.array_equal(a[:n * w].cpu().numpy().view(np.uint32), b[:n * w].cpu().numpy().view(np.uint32))
        assert len(moved.packed()) == (2 if z_spread else 1)
        a, b = moved.row_data()[0][0], fresh.row_data()[0][0]
        assert np.array_equal(a[:4 * n].cpu().numpy().view(np.uint32), b[:4 * n].cpu().numpy().view(np.uint32))
    finally:
        moved.close()
        fresh.close()
