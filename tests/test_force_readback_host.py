"""CPU tests of ``P.check_force_from_velocity``, the force read back through one uncapped velocity update (dt = 1,
max_speed_factor = 1e4) that the GPU tests of the fused tick and the batch kernel -- neither can record its forces -- rely on.

A fake device result v' = fp32(v + dt fp32(F)) built from the NumPy oracle's forces on a realistic 200-pedestrian crowd must pass
unperturbed and fail for each injected error: one row's pedestrian force scaled by 1 + 1e-4, one row missing its nearest
neighbour's term, that term counted twice, F_z dropped in 3-D.  Each test also prints what ``P.check_velocity`` at dt = 0.05 with
the speed cap on says about the same error (the bound of the older v'-only tests of these kernels)."""
import numpy as np
import pytest

import _parity as P
from carla_social_force_model_amd import scenarios
from carla_social_force_model_amd.config import default_sfm_config
from oracle import sfm_oracle as O

N = 200
MSF = 1e4           # max_speed_factor of the readback ticks: the cap cannot act


def _crowd(z_spread):
    sc = scenarios.make_scenario(N, 7100, density=1.0, z_spread=z_spread)
    cfg = default_sfm_config(("pedestrian_force",))
    prm = O.OracleParams.from_config(cfg)
    diag = {}
    with np.errstate(all="ignore"):
        _, F, _ = O.tick_forces(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, np.zeros(N, bool), O.Geometry(), prm,
                                theta_tol=P.THETA_TOL, tie_rel=P.TIE_REL, diag=diag)
    expo, absum = diag["total"]
    return sc, prm, F, expo, absum


def _fake_device(vel, F, dt, max_speed=None):
    """fp32 forces, one fp32 update (and the fp32 cap when ``max_speed`` is given), as a kernel computes them."""
    F32 = np.float32(F).astype(np.float64)
    v = vel + dt * F32
    if max_speed is not None:
        v = O.cap_velocity(v, max_speed)
    return np.float32(v).astype(np.float64)


def _check(sc, F_dev, F_ref, expo, absum):
    return P.check_force_from_velocity("pedestrian", _fake_device(sc.vel, F_dev, 1.0), sc.vel, 1.0, F_ref, absum, expo,
                                       sc.target_speed * MSF)


def _old_check_says(sc, F_dev, F_ref, expo):
    """What check_velocity at dt = 0.05, cap on (max_speed_factor 1.3), makes of the same device forces."""
    ms = sc.target_speed * 1.3
    v_ref = O.new_velocities(sc.vel, F_ref, sc.target_speed, 0.05)
    try:
        P.check_velocity(_fake_device(sc.vel, F_dev, 0.05, ms), v_ref, expo, 0.05)
        return "passes (the error is missed)"
    except AssertionError:
        return "fails (the error is caught)"


def _probe_row(F, expo, absum):
    """The row where the per-force bound is tightest: no exposure, largest |F| / A."""
    rel = np.linalg.norm(F, axis=1) / np.maximum(absum, 1e-300)
    rel[(expo > 0) | ~np.isfinite(rel)] = -1.0
    i = int(np.argmax(rel))
    assert rel[i] > 0.1, rel[i]
    return i


def _nearest_term(sc, prm, i):
    """f_ij of row i's nearest neighbour j (the pedestrian force of a two-body crowd {i, j} on i)."""
    d = np.linalg.norm(sc.loc - sc.loc[i], axis=1)
    d[i] = np.inf
    j = int(np.argmin(d))
    f, _, _ = O.pedestrian_force(sc.loc[[i, j]], sc.vel[[i, j]], sc.radius[[i, j]], prm.ped, prm.use_ped_radius)
    return f[0]


def _nearest_probe_row(sc, prm, expo, absum):
    """(row i, f_ij of its nearest neighbour) for the row without exposure whose nearest neighbour's term is the largest part of
    A_i (a neighbour behind the pedestrian contributes next to nothing -- exp(-(n B theta)^2) -- and dropping it is no error)."""
    terms = np.array([_nearest_term(sc, prm, i) for i in range(N)])
    rel = np.linalg.norm(terms, axis=1) / np.maximum(absum, 1e-300)
    rel[expo > 0] = -1.0
    i = int(np.argmax(rel))
    assert rel[i] > 0.1, rel[i]
    return i, terms[i]


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
def test_unperturbed_forces_pass(z_spread):
    sc, _, F, expo, absum = _crowd(z_spread)
    worst, floor_rows = _check(sc, F, F, expo, absum)
    print(f"\nunperturbed ({'3-D' if z_spread else 'planar'}): worst |dF|/max(|F|,A) {worst:.2e}, {floor_rows} of {N} rows needed "
          f"the fp32 floor")
    assert worst < 1e-5


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
@pytest.mark.parametrize("kind", ["scaled_1e-4", "nearest_missing", "nearest_twice"])
def test_injected_errors_are_rejected(kind, z_spread):
    sc, prm, F, expo, absum = _crowd(z_spread)
    bad = F.copy()
    if kind == "scaled_1e-4":
        i = _probe_row(F, expo, absum)
        bad[i] *= 1.0 + 1e-4
    else:
        i, f_ij = _nearest_probe_row(sc, prm, expo, absum)
        bad[i] += -f_ij if kind == "nearest_missing" else f_ij
    with pytest.raises(AssertionError, match="out of tolerance"):
        _check(sc, bad, F, expo, absum)
    print(f"\n{kind} ({'3-D' if z_spread else 'planar'}), row {i} (|F| {np.linalg.norm(F[i]):.3g}, A {absum[i]:.3g}, "
          f"|dF| {np.linalg.norm(bad[i] - F[i]):.3g}): readback rejects it; check_velocity at dt = 0.05 "
          f"{_old_check_says(sc, bad, F, expo)}")


def test_dropped_z_component_is_rejected():
    sc, _, F, expo, absum = _crowd(1.5)
    bad = F.copy()
    bad[:, 2] = 0.0
    with pytest.raises(AssertionError, match="out of tolerance"):
        _check(sc, bad, F, expo, absum)
    print(f"\nF_z = 0 (3-D): readback rejects it; check_velocity at dt = 0.05 {_old_check_says(sc, bad, F, expo)}")


def test_a_row_near_the_cap_is_refused():
    """The readback is only meaningful while the cap cannot act: a reference v' within a factor of 10 of it is an error of the test."""
    sc, _, F, expo, absum = _crowd(0.0)
    with pytest.raises(AssertionError, match="speed cap"):
        P.check_force_from_velocity("pedestrian", _fake_device(sc.vel, F, 1.0), sc.vel, 1.0, F, absum, expo, sc.target_speed * 1.3)


def test_nan_rows_must_agree():
    sc, _, F, expo, absum = _crowd(0.0)
    v = _fake_device(sc.vel, F, 1.0)
    v[3] = np.nan
    with pytest.raises(AssertionError, match="NaN rows differ"):
        P.check_force_from_velocity("pedestrian", v, sc.vel, 1.0, F, absum, expo, sc.target_speed * MSF)
