"""The oracle alone must make tests/test_encounters_gpu.py meaningful (CPU only; tests/_encounters.py says what the crowds are).

For EVERY crowd the GPU file builds (``_encounters.crowd_specs()``: both files read the same list), stock parameters, forces
("pedestrian_force",), use_ped_radius both ways, ``c_oracle.tick(..., theta_tol=P.THETA_TOL, plain=...)``:
  * a row QUALIFIES when its term is >= 1e-3 m/s^2, its exposure is zero and its conditioning weight absum / plain - 1 is <= 1:
    at least 50 % of the paired rows qualify, at most 10 % carry a non-zero exposure;
  * every bin of the grid (8 octants of the angle between e and t x 3 distance bands x 2 bands of |D|) that the oracle's formula
    can fill at all holds >= 4 qualifying rows in every crowd of >= 1024 pairs; the six bins in which no grid point of the formula
    qualifies (``feasible_bins``: |D| >= 2 with the partner behind; largest term 2.1e-4 m/s^2) hold >= 4 checked rows;
  * on the qualifying rows the plain formula in NumPy float32 stays within HALF of ``check_force``'s allowance of the float64 term,
    and with its two norms up to one ulp off within the allowance on every paired row.
Measured (crowds of >= 1024 pairs, every matching, both radius settings): qualifying 77-82 % of the paired rows, exposed 0.5-0.9 %,
median term 0.017-0.1 m/s^2, rows with weight > 1: 9-11 %; float32 formula against the allowance: worst 0.44, with the norms one ulp
off 0.59 (every crowd prints its own with -s).  Small crowds: qualifying 56-100 %, exposed up to 4.7 %.
"""
import functools

import numpy as np
import pytest

import _encounters as E
import _param_sets as psets
import _parity as P
from oracle import c_oracle
from oracle import sfm_oracle as O

SPECS = E.crowd_specs()


def _id(spec):
    n, m, seed, z, layout = spec
    return f"{n}-{m}-{'3d' if z else 'planar'}-{layout}"


@functools.lru_cache(maxsize=None)
def _cfg(rad):
    return psets.config("stock", E.PED_ONLY, use_ped_radius=rad)


@pytest.mark.parametrize("spec", SPECS, ids=[_id(s) for s in SPECS])
def test_oracle_side_conditions(spec):
    n, m, seed, z, layout = spec
    crowd = E.isolated_pairs(n, m, seed, z, layout)
    pr = crowd.paired
    assert pr.sum() == 2 * crowd.n_pairs and (crowd.partner[crowd.partner[pr]] == np.nonzero(pr)[0]).all()     # a perfect matching
    assert np.array_equal(crowd.sc.loc, E._f32(crowd.sc.loc)) and np.array_equal(crowd.sc.vel, E._f32(crowd.sc.vel))
    for rad in (False, True):
        ref = E.reference(crowd, _cfg(rad))
        label = f"{_id(spec)} rad={rad}"
        exposed = (np.nan_to_num(ref.expo[pr]) > 0).sum()
        assert ref.qualifying.sum() >= 0.5 * pr.sum(), (label, ref.qualifying.sum(), pr.sum())
        assert exposed <= 0.10 * pr.sum(), (label, exposed)
        if crowd.n_pairs >= 1024:
            E.assert_bins(label, ref)
        # the reference alone: a plain float32 evaluation uses at most half of the allowance
        err = np.linalg.norm(E.plain_float32_term(crowd, rad) - ref.F, axis=1)
        ratio = err[ref.qualifying] / E.allowance(ref)[ref.qualifying]
        print(f"\n{label}: pairs {crowd.n_pairs}  qualifying {ref.qualifying.sum()}  exposed {exposed}  median term "
              f"{np.median(ref.term[pr]):.3g}  weight > 1: {(ref.weight[pr] > 1).mean():.1%}  float32 formula / allowance {ratio.max():.3f}")
        assert ratio.max() <= 0.5, (label, ratio.max())
        # ... and with its two norms up to one ulp off (a 1-ulp reciprocal square root) it stays inside the allowance on EVERY row
        if m in (1, "random"):                               # (the encounters are the same under every matching)
            worst = 0.0
            for nudge in ((-1, -1), (-1, 1), (1, -1), (1, 1), (0, 1), (1, 0), (0, -1), (-1, 0)):
                err = np.nan_to_num(np.linalg.norm(E.plain_float32_term(crowd, rad, nudge=nudge) - ref.F, axis=1))
                worst = max(worst, float(np.max(err[pr] / E.allowance(ref)[pr])))
            print(f"    norms one ulp off: worst err / allowance over all paired rows {worst:.3f}")
            assert worst <= 1.0, (label, worst)


def test_feasible_bins_table():
    """Which bins the formula can fill (printed with -s): a bin is written off only when its largest term stays below QUALIFY_TERM."""
    for rad in (False, True):
        best, share, feasible = E.feasible_bins(rad)
        print(f"\nuse_ped_radius={rad}: largest term / share of the bin that qualifies, rows = octants from -pi, columns = "
              f"(0.3-0.7, 0.7-1.5, 1.5-3 m) x (|D| < 2, >= 2)")
        for o in range(8):
            print("   " + "  ".join(f"{best[o * 6 + k]:9.2e}/{share[o * 6 + k]:6.4f}" for k in range(6)))
        assert np.nonzero(~feasible)[0].tolist() == [1, 3, 5, 43, 45, 47]
        assert (best[~feasible] < 0.25 * E.QUALIFY_TERM).all() and (best[feasible] >= 3.0 * E.QUALIFY_TERM).all()


@pytest.mark.parametrize("z", [0.0, 1.5], ids=["planar", "3d"])
@pytest.mark.parametrize("rad", [False, True], ids=["norad", "rad"])
def test_c_oracle_against_numpy_oracle(z, rad):
    """One crowd, both oracles: the same forces, NaN / inf in the same places; the B = 0 encounters come out exactly 0.0."""
    crowd = E.isolated_pairs(300, 33, E.SEED + 300, z)
    sc = crowd.sc
    ref = E.reference(crowd, _cfg(rad))
    with np.errstate(all="ignore"):
        F, expo, absum = O.pedestrian_force(sc.loc, sc.vel, sc.radius, E.STOCK, rad, theta_tol=P.THETA_TOL)
    assert np.array_equal(np.isnan(F), np.isnan(ref.F)) and np.array_equal(np.isinf(F), np.isinf(ref.F))
    assert np.isfinite(ref.F).all()
    P.check_force("C oracle vs NumPy oracle", ref.F, F, absum, expo, rtol=1e-12)
    assert np.allclose(np.nan_to_num(ref.expo), np.nan_to_num(expo), rtol=1e-9, atol=0)
    # (the scale: the C oracle leaves NaN where a term's conditioning weight is 0 / 0 -- the B = 0 rows among them -- where the
    #  NumPy oracle skips the term; check_force reads a NaN scale as 0, and those rows' own check is ``== 0`` anyway)
    fin = np.isfinite(ref.absum)
    a_rows = sorted(r for k, rows in crowd.designed.items() if k.startswith("a:") for r in rows)
    # (... and on one side of two other designed encounters -- "b:-e,d=2" on the wrap, "d:steep" -- where an exponential underflows
    #  to 0 while its weight overflows; never on a drawn encounter, never on a qualifying row)
    other = {r for k, rows in crowd.designed.items() if k in ("b:-e,d=2", "d:steep") for r in rows}
    nan_rows = set(np.nonzero(~fin)[0].tolist())
    assert set(a_rows) <= nan_rows and nan_rows - set(a_rows) <= other and not ref.qualifying[~fin].any()
    assert np.allclose(ref.absum[fin], absum[fin], rtol=1e-9, atol=1e-300)
    for label, rows in crowd.designed.items():
        if not label.startswith("a:"):
            continue
        # the partner's term alone (the row's sum also holds ~1e-40 m/s^2 from 100 m away): the pair as a crowd of two
        two = np.array(rows)
        prm = O.OracleParams.from_config(_cfg(rad))
        with np.errstate(all="ignore"):
            per, _, _, ex, _ = c_oracle.tick(sc.loc[two], sc.vel[two], sc.waypoint[two], sc.target_speed[two], sc.radius[two],
                                             np.zeros(2, bool), O.Geometry(), prm, 1.0, theta_tol=P.THETA_TOL)
            Fn, _, _ = O.pedestrian_force(sc.loc[two], sc.vel[two], sc.radius[two], E.STOCK, rad)
        assert (per["pedestrian_force"] == 0.0).all() and (Fn == 0.0).all() and (ex == 0.0).all(), (label, per["pedestrian_force"], Fn)
        assert (np.abs(ref.F[two]) <= 1e-12).all()


def test_matchings_hold_the_same_encounters():
    """Two matchings of one crowd: the same pairs of states at different indices."""
    a, b = E.isolated_pairs(1024, 64, E.SEED + 1024), E.isolated_pairs(1024, "random", E.SEED + 1024)
    ia, ib = a.ident(), b.ident()
    assert np.array_equal(np.sort(ia), np.sort(ib)) and not np.array_equal(ia, ib)
    oa, ob = np.argsort(ia), np.argsort(ib)
    for k in ("loc", "vel", "radius"):
        assert np.array_equal(getattr(a.sc, k)[oa], getattr(b.sc, k)[ob])


def test_index_maps_on_small_cases():
    """The index maps of ``_encounters`` against hand-worked slots (csrc/sfm_kernels.hip, lines cited in their docstrings)."""
    # symmetric kernel, n_t = 4: tiles 0 and 3 are one apart going up from 3 -> tile 3 travels, shift 1; lanes 5 (tile 0), 9 (tile 3)
    shift, sigma, wave, step = E.slots_symmetric(256, [5], [3 * 64 + 9])
    assert (shift[0], sigma[0], wave[0], step[0]) == (1, 4, 0, 4)
    # ... antipodal tiles 0 and 2: the lower tile travels; resident lane 9 meets travelling lane 5 at sigma = 60: wave 3, step 12
    shift, sigma, wave, step = E.slots_symmetric(256, [5], [2 * 64 + 9])
    assert (shift[0], sigma[0], wave[0], step[0]) == (2, 60, 3, 12)
    # diagonal tile: lanes 3 and 40, delta 37 > 32 -> sigma 27: wave 1 (17..32), step 10
    shift, sigma, wave, step = E.slots_symmetric(256, [3], [40])
    assert (shift[0], sigma[0], wave[0], step[0]) == (0, 27, 1, 10)
    # fused tick, 16 waves: same pair on a diagonal tile -> chain B (17..32) of the first wave pair: r = 26, XB = 16: chain 1, wave 1, step 2
    kind, shift, sigma, wave, chain, step = E.slots_fused(256, [3], [40], 16)
    assert (kind[0], sigma[0], wave[0], chain[0], step[0]) == (0, 27, 1, 1, 2)
    # ... tile 0 past tile 1 of a group: resident lane 9 of tile 1 meets lane 5 of tile 0 at sigma 60: chain B, (60 - 32) = 28: wave 3, step 4
    kind, shift, sigma, wave, chain, step = E.slots_fused(256, [5], [64 + 9], 16)
    assert (kind[0], shift[0], sigma[0], wave[0], chain[0], step[0]) == (1, 1, 60, 3, 1, 4)
    # ... 8 waves: HALF = 16 double steps, two waves per tile pair
    kind, shift, sigma, wave, chain, step = E.slots_fused(256, [5], [64 + 9], 8)
    assert (wave[0], chain[0], step[0]) == (1, 1, 12)
    assert E.fused_waves(4096, False) == 16 and E.fused_waves(4096, True) == 8 and E.fused_waves(256, True) == 16
    assert E.slots_batch(64, [3], [40]) == (4, 2, 0) and E.slots_batch(300, [299], [3])[2] == 1


@pytest.mark.parametrize("path,n,z,rad,layout", [p for p in E.PATHS if p[0] != "list"], ids=[f"{p[0]}-{p[1]}-{'3d' if p[2] else 'planar'}-{'rad' if p[3] else 'norad'}" for p in E.PATHS if p[0] != "list"])
def test_slot_coverage_of_a_path(path, n, z, rad, layout):
    """Over a path's matchings every slot carries a qualifying term (``_encounters.assert_coverage``; the GPU file asserts the same
    before it runs the cells)."""
    print("\n" + E.assert_coverage(path, n, z, rad, layout, _cfg(rad)))
