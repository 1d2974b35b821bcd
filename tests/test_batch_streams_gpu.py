"""GPU tests of the batch's waypoint streams and recorded runs (sfm_batch_set_waypoint_streams, sfm_batch_download_waypoints,
sfm_batch_run_recorded; SfmBatch.set_waypoint_streams / waypoints / run_recorded, tick(redraw=True) / run(redraw=True)):
redraws against the oracle every tick, recorded frames against step-wise downloads, batch invariance with streams on, uploads
resetting the draw counters, and refused arguments.  Run on the MI355X box with  python -m pytest tests -m gpu."""
import ctypes as C

import numpy as np
import pytest

import _parity as P
from carla_social_force_model_amd import _lib, scenarios
from carla_social_force_model_amd.batch import SfmBatch
from carla_social_force_model_amd.config import default_sfm_config
from oracle import sfm_oracle as O

pytestmark = pytest.mark.gpu

PED = ("acceleration_force", "pedestrian_force")
BORDERS = ("acceleration_force", "pedestrian_force", "border_force")


def _scene(n, seed, z_spread=0.0, borders=0, static=0, dynamic=0, crossing=False):
    sc = vars(scenarios.make_scenario(n, seed, n_borders=borders, n_static=static, n_dynamic=dynamic, z_spread=z_spread,
                                      border_len=(3.0, 15.0)))
    rng = np.random.default_rng(seed + 17)
    sc["radius"] = np.float32(rng.uniform(0.2, 0.45, n)).astype(np.float64)
    sc["dynamic_vel"] = sc["dynamic_vel"] * 0.1          # slow vehicles: the plain 1e-5 bound on v' holds
    if crossing:
        sc["crossing"] = rng.random(n) < 0.2
    return sc


def _config(k, forces):
    cfg = default_sfm_config(forces)
    cfg["pedestrian_force"].update({"A": 3.0 + 0.5 * k, "lambda": 1.5 + 0.1 * k})
    cfg["goal_force"] = {"tau": 0.4 + 0.05 * k}
    cfg["use_ped_radius"] = bool(k % 2)
    return cfg


def _mixed(z_spread):
    """Scenes, configs, step lengths and streams (seed, side, threshold) of the redraw tests: N = 64 with all five forces, 200 with
    a crossing mask and borders (a small side: frequent arrivals), 1 (starting next to its waypoint), 0 and 1024."""
    scenes = [_scene(64, 801, z_spread, borders=4, static=2, dynamic=2), _scene(200, 802, z_spread, borders=6, crossing=True),
              _scene(1, 803, z_spread), _scene(0, 804, z_spread), _scene(1024, 805, z_spread)]
    scenes[2]["waypoint"][0, :2] = scenes[2]["loc"][0, :2] + np.array([0.5, 0.0])
    cfgs = [_config(0, scenarios.ALL_FORCES), _config(1, BORDERS), _config(2, PED), _config(3, PED), _config(4, PED)]
    dts = [0.05, 0.04, 0.05, 0.05, 0.05]
    ws = [sc["world_side"] for sc in scenes]
    seeds = [11, 0xDEADBEEF, 7, 3, 123456]
    sides = [ws[0], 0.2 * ws[1], ws[2], ws[3], ws[4]]
    thrs = [3.0, 2.5, 2.0, 2.0, 4.0]
    return scenes, cfgs, dts, (seeds, sides, thrs)


def _batch(scenes, cfgs, dts, streams=None):
    b = SfmBatch(cfgs, dts)
    b.upload(scenes)
    if streams is not None:
        b.set_waypoint_streams(*streams)
    return b


def _everything(b):
    """State, waypoints and draw counters of every scene (bitwise comparable)."""
    return [(loc, vel, wp, dr) for (loc, vel), (wp, dr) in zip(b.state(), b.waypoints())]


def _assert_same(xs, ys, what):
    assert len(xs) == len(ys)
    for k, (x, y) in enumerate(zip(xs, ys)):
        for q, (u, v) in enumerate(zip(x, y)):
            assert u.shape == v.shape and np.array_equal(u, v), f"{what}: scene {k}, field {q}"


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_redraw_matches_the_oracle_every_tick(z_spread):
    """30 ticks of tick(integrate=True, redraw=True), every tick re-synchronised against O.free_step from the device's fp32 state:
    v' (1e-5), x' (1e-6), draw counters equal, redrawn waypoints bitwise O.redraw_waypoint(scene-local index, draws, seed, side).
    Only a pedestrian whose distance^2 to its waypoint lies within 1e-5 relative of thr^2 is exempt from the arrival checks."""
    scenes, cfgs, dts, (seeds, sides, thrs) = _mixed(z_spread)
    b = _batch(scenes, cfgs, dts, (seeds, sides, thrs))
    try:
        assert b.planar == (z_spread == 0.0)
        cur = []
        for sc, (wp, dr) in zip(scenes, b.waypoints()):
            assert not dr.any()
            cur.append((np.float32(sc["loc"]).astype(np.float64), np.float32(sc["vel"]).astype(np.float64), wp.copy(), dr.copy()))
        total_draws = 0
        for t in range(30):
            b.tick(integrate=True, redraw=True)
            got = _everything(b)
            for k, (sc, cfg, dt) in enumerate(zip(scenes, cfgs, dts)):
                n = len(sc["loc"])
                if n == 0:
                    continue
                loc, vel, wp, draws = cur[k]
                wp3 = np.zeros((n, 3))
                wp3[:, :2] = wp
                prm = O.OracleParams.from_config(cfg)
                geom = O.Geometry(sc["borders"], sc["border_centers"], sc["border_lengths"], sc["static_obstacles"],
                                  sc["dynamic_obstacles"], sc["dynamic_vel"])
                crossing = sc.get("crossing")
                crossing = np.zeros(n, bool) if crossing is None else crossing
                with np.errstate(all="ignore"):
                    oloc, ovel, owp, odraws = O.free_step(loc, vel, wp3, sc["target_speed"], sc["radius"], crossing,
                                                          draws.astype(np.int64), geom, prm, dt, arrive_threshold=thrs[k],
                                                          seed=seeds[k], world_side=sides[k], redraw=True, round_f32=True)
                    diag = {}
                    O.tick_forces(loc, vel, wp3, sc["target_speed"], sc["radius"], crossing, geom, prm,
                                  theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
                dloc, dvel, dwp, ddraws = got[k]
                P.check_velocity(dvel, ovel, diag["total"][0], dt)
                assert np.max(np.abs(dloc - oloc)) <= 1e-6 * max(1.0, np.max(np.abs(oloc))) + 1e-6, f"scene {k} tick {t}"
                # arrival on the pre-move position against this tick's waypoint, in the device's fp32 threshold
                d2 = np.sum((wp - loc[:, :2]) ** 2, axis=1)
                thr2 = float(np.float32(np.float64(thrs[k]) ** 2))
                sure = np.abs(d2 - thr2) > 1e-5 * thr2
                assert np.array_equal(ddraws[sure].astype(np.int64), odraws[sure]), f"draw counters: scene {k} tick {t}"
                hit = sure & (odraws > draws)
                ids = np.nonzero(hit)[0]
                if ids.size:
                    want = O.redraw_waypoint(ids, ddraws[ids], seeds[k], sides[k])
                    assert np.array_equal(dwp[ids], want), f"redrawn waypoints: scene {k} tick {t}"
                    assert np.array_equal(np.float32(owp[ids, :2]), want)
                kept = sure & ~hit
                assert np.array_equal(dwp[kept], wp[kept]), f"kept waypoints: scene {k} tick {t}"
                total_draws += int((ddraws.astype(np.int64) - draws).sum())
                cur[k] = (dloc, dvel, dwp.copy(), ddraws.astype(np.int64))     # continue from the device
        assert total_draws >= 20, f"only {total_draws} redraws in 30 ticks: the redraw branch was hardly exercised"
    finally:
        b.close()


def _recording_scenes(z_spread):
    scenes = [_scene(64, 901, z_spread, borders=4, static=2, dynamic=2), _scene(200, 902, z_spread, borders=6, crossing=True),
              _scene(0, 903, z_spread), _scene(17, 904, z_spread)]
    cfgs = [_config(0, scenarios.ALL_FORCES), _config(1, BORDERS), _config(2, PED), _config(3, PED)]
    dts = [0.05, 0.04, 0.05, 0.02]
    streams = ([5, 6, 7, 8], [sc["world_side"] for sc in scenes], [3.0, 4.0, 2.0, 5.0])
    return scenes, cfgs, dts, streams


@pytest.mark.parametrize("redraw", [False, True], ids=["plain", "redraw"])
@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_recorded_frames_equal_stepwise_downloads(z_spread, redraw):
    """A.run_recorded(9, stride=4) against B stepped with run(4), run(4), run(1) and a download before each: frames bitwise equal,
    ticks_idx [0, 4, 8], the same final state, waypoints and draw counters.  max_frames=2 keeps 2 frames and still runs 9 ticks;
    ticks=0 gives no frame and changes nothing."""
    scenes, cfgs, dts, streams = _recording_scenes(z_spread)
    A, B_, Cb = (_batch(scenes, cfgs, dts, streams) for _ in range(3))
    try:
        frames, idx, zframes = A.run_recorded(9, stride=4, redraw=redraw)
        assert list(idx) == [0, 4, 8]
        assert (zframes is None) == (z_spread == 0.0)
        want = [[] for _ in scenes]
        for k in (0, 4, 8):
            for s, (loc, vel) in enumerate(B_.state()):
                want[s].append((np.float32(np.concatenate([loc[:, :2], vel[:, :2]], axis=1)),
                                np.float32(np.stack([loc[:, 2], vel[:, 2]], axis=1))))
            B_.run(min(4, 9 - k), redraw=redraw)
        for s, sc in enumerate(scenes):
            n = len(sc["loc"])
            assert frames[s].shape == (3, n, 4) and frames[s].dtype == np.float32
            assert np.array_equal(frames[s], np.stack([w[0] for w in want[s]]).reshape(3, n, 4)), f"scene {s}: frames"
            if zframes is not None:
                assert zframes[s].shape == (3, n, 2)
                assert np.array_equal(zframes[s], np.stack([w[1] for w in want[s]]).reshape(3, n, 2)), f"scene {s}: zframes"
        final = _everything(B_)
        _assert_same(_everything(A), final, "run_recorded vs run")
        if redraw:
            assert sum(int(dr.sum()) for _, _, _, dr in final) > 0, "no redraw happened"

        f2, idx2, z2 = Cb.run_recorded(9, stride=4, redraw=redraw, max_frames=2)
        assert list(idx2) == [0, 4] and all(f.shape[0] == 2 for f in f2)
        assert all(np.array_equal(f2[s], frames[s][:2]) for s in range(len(scenes)))
        if z2 is not None:
            assert all(np.array_equal(z2[s], zframes[s][:2]) for s in range(len(scenes)))
        _assert_same(_everything(Cb), final, "max_frames=2 still runs every tick")

        f0, idx0, z0 = Cb.run_recorded(0, stride=4, redraw=redraw)
        assert len(idx0) == 0 and all(f.shape[0] == 0 for f in f0)
        _assert_same(_everything(Cb), final, "ticks=0 changes nothing")
    finally:
        for b in (A, B_, Cb):
            b.close()


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_scene_is_independent_of_the_batch_with_streams_on(z_spread):
    """A scene's frames, waypoints and draw counters are bitwise the same alone and at position 3 of a batch of 7 mixed scenes
    (every scene with its own stream), over 12 redrawing ticks."""
    target = _scene(65, 77, z_spread, borders=4, static=2, crossing=True)
    tcfg, tdt, tstream = _config(3, scenarios.ALL_FORCES), 0.04, (99, 0.3 * target["world_side"], 4.0)
    others = [_scene(n, 1000 + k, z_spread, borders=3 if k % 2 else 0) for k, n in enumerate((30, 0, 130, 1, 64, 250))]
    ocfgs = [_config(k, BORDERS if k % 2 else PED) for k in range(6)]
    scenes = others[:3] + [target] + others[3:]
    cfgs = ocfgs[:3] + [tcfg] + ocfgs[3:]
    dts = [0.05] * 3 + [tdt] + [0.05] * 3
    streams = ([1, 2, 3, tstream[0], 4, 5, 6], [sc["world_side"] for sc in others[:3]] + [tstream[1]] +
               [sc["world_side"] for sc in others[3:]], [3.0, 2.0, 2.5, tstream[2], 3.5, 2.0, 3.0])
    alone = _batch([target], [tcfg], [tdt], ([tstream[0]], [tstream[1]], [tstream[2]]))
    mixed = _batch(scenes, cfgs, dts, streams)
    try:
        fa, _, za = alone.run_recorded(12, stride=3, redraw=True)
        fm, _, zm = mixed.run_recorded(12, stride=3, redraw=True)
        assert np.array_equal(fa[0], fm[3])
        if za is not None:
            assert np.array_equal(za[0], zm[3])
        ea, em = _everything(alone), _everything(mixed)
        _assert_same(ea, em[3:4], "alone vs position 3")
        assert ea[0][3].sum() > 0, "the scene never redrew"
    finally:
        alone.close()
        mixed.close()


def test_upload_resets_draws_and_keeps_the_streams():
    """After run(10, redraw=True) an upload zeroes every draw counter and restores the uploaded waypoints; the streams stay set
    (also across set_params), so the same run again gives the same bits."""
    scenes, cfgs, dts, streams = _mixed(0.0)
    b = _batch(scenes, cfgs, dts, streams)
    try:
        b.run(10, redraw=True)
        first = _everything(b)
        assert sum(int(e[3].sum()) for e in first) > 0
        b.upload(scenes)
        for sc, (wp, dr) in zip(scenes, b.waypoints()):
            assert dr.dtype == np.uint32 and not dr.any()
            assert np.array_equal(wp, np.float32(sc["waypoint"][:, :2]))
        b.set_params(cfgs, dts)
        b.run(10, redraw=True)
        _assert_same(_everything(b), first, "second run after the upload")
    finally:
        b.close()


def test_refusals_leave_the_batch_usable():
    """Every refused argument of the new calls, and redraw before the streams are set: nothing is launched (the state is bitwise
    unchanged), and a valid tick works afterwards."""
    L = _lib.load()
    scenes = [_scene(5, 1), _scene(3, 2)]
    b = SfmBatch([_config(0, PED), _config(1, PED)], [0.05, 0.05])
    try:
        b.upload(scenes)
        h = b._b

        def err():
            return L.sfm_batch_last_error(h).decode()

        before = _everything(b)
        # redraw before any stream is set: refused, the message names the flag a batch does take
        for call in (lambda: b.tick(integrate=True, redraw=True), lambda: b.run(2, redraw=True),
                     lambda: b.run_recorded(2, redraw=True)):
            with pytest.raises(_lib.SfmLibraryError, match="SFM_TICK_INTEGRATE"):
                call()
        seed = np.array([1, 2], np.uint32)
        side = np.array([10.0, 10.0], np.float32)
        thr = np.array([2.0, 2.0], np.float32)
        bad_side = np.array([10.0, -1.0], np.float32)
        nan_thr = np.array([np.nan, 2.0], np.float32)
        inf_side = np.array([np.inf, 1.0], np.float32)
        neg_thr = np.array([2.0, -0.5], np.float32)
        p = lambda a: a.ctypes.data
        assert L.sfm_batch_set_waypoint_streams(h, None, p(side), p(thr)) != 0 and "NULL" in err()
        assert L.sfm_batch_set_waypoint_streams(h, p(seed), None, p(thr)) != 0 and "NULL" in err()
        assert L.sfm_batch_set_waypoint_streams(h, p(seed), p(side), None) != 0 and "NULL" in err()
        for s_, t_ in ((bad_side, thr), (inf_side, thr), (side, nan_thr), (side, neg_thr)):
            assert L.sfm_batch_set_waypoint_streams(h, p(seed), p(s_), p(t_)) != 0 and "finite" in err()
        with pytest.raises(_lib.SfmLibraryError, match="SFM_TICK_INTEGRATE"):
            b.tick(integrate=True, redraw=True)           # the refused stream calls set nothing

        frames = np.zeros((4, 8, 4), np.float32)
        zf = np.zeros((4, 8, 2), np.float32)
        nf = C.c_int(-7)
        rr = lambda ticks, flags, stride, fr, z, mf, n=C.byref(nf): L.sfm_batch_run_recorded(h, ticks, flags, stride, fr, z, mf, n)
        assert rr(-1, 0, 1, p(frames), None, 4) != 0
        assert rr(4, 0, 0, p(frames), None, 4) != 0
        assert rr(4, 0, -2, p(frames), None, 4) != 0
        assert rr(4, 0, 1, p(frames), None, -1) != 0
        assert rr(4, 0, 1, None, None, 4) != 0 and "frames is NULL" in err()
        assert rr(4, 0, 1, p(frames), None, 4, None) != 0 and "n_frames" in err()
        assert rr(4, 0, 1, p(frames), p(zf), 4) != 0 and "planar" in err()
        assert rr(4, _lib.TICK_RECORD_FORCES, 1, p(frames), None, 4) != 0 and "SFM_TICK_INTEGRATE" in err()
        assert rr(4, _lib.TICK_REDRAW_WAYPOINTS, 1, p(frames), None, 4) != 0 and "SFM_TICK_INTEGRATE" in err()
        # more frame bytes than one call may record (8 rows x 16 bytes x 9e6 frames > 1 GiB): refused before anything runs
        assert rr(9_000_000, 0, 1, p(frames), None, 9_000_000) != 0 and "split" in err()
        _assert_same(_everything(b), before, "state after the refused calls")

        # valid calls still work: streams, then a redrawing tick and a recorded run
        b.set_waypoint_streams([1, 2], 10.0, 2.0)
        b.tick(integrate=True, redraw=True)
        fr, idx, zfr = b.run_recorded(3, stride=2, redraw=True)
        assert list(idx) == [0, 2] and zfr is None and fr[0].shape == (2, 5, 4) and fr[1].shape == (2, 3, 4)
        assert all(np.isfinite(v).all() for _, v in b.state())
        # after streams are set, flags other than INTEGRATE / REDRAW are still refused
        with pytest.raises(_lib.SfmLibraryError, match="SFM_TICK_INTEGRATE"):
            b._check(L.sfm_batch_tick(h, _lib.TICK_RECORD_FORCES), "sfm_batch_tick")
    finally:
        b.close()
