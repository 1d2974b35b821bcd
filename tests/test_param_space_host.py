"""CPU side of the parameter-space tests (tests/_param_sets.py): what has to hold on the ORACLE ALONE before a GPU cell of
tests/test_param_space_gpu.py means anything.

  * the C oracle, which the large GPU cells lean on, against the NumPy oracle at every set (the reference fixtures stop at N = 64):
    all forces, planar and 3-D, at the gate tests/test_oracle_golden.py applies (1e-12 of the largest value);
  * the two conditions of tests/_param_cells.py on the scenarios the GPU cells use: exposed rows <= 10 %, max_amp <= 1;
  * the list cutoff has something to lose: at longrange a reach built from the STOCK gamma / lambda would drop terms whose
    float64 sum exceeds check_force's allowance for at least 1 % of the rows."""
import numpy as np
import pytest

import _param_cells as pc
import _param_sets as psets
import _parity as P
from carla_social_force_model_amd import scenarios
from oracle import c_oracle
from oracle import sfm_oracle as O
from test_oracle_golden import _close

SETS = psets.NAMES + ("integrate_fine",)


def test_every_set_moves_what_it_says():
    stock = psets.config("stock")
    for name in SETS:
        cfg = psets.config(name)
        assert cfg != stock and cfg["forces"] == stock["forces"], name
    p = O.OracleParams.from_config(psets.config("integrate"))
    assert (p.tau, p.max_speed_factor, psets.step_of("integrate"), psets.step_of("integrate_fine")) == (0.25, 2.0, 0.1, 0.0125)
    p = O.OracleParams.from_config(psets.config("lam0"))
    assert p.ped.lam == 0.0 and p.static.lam == 0.0 and p.static.perception_threshold == 7 and p.dynamic.perception_threshold == 11


@pytest.mark.parametrize("z_spread", [0.0, 1.5], ids=["planar", "3d"])
@pytest.mark.parametrize("rad", [False, True], ids=["plain", "radius"])
@pytest.mark.parametrize("name", SETS)
def test_c_oracle_matches_numpy_oracle(name, rad, z_spread):
    n = 384
    sc = pc.scene(n, 4300, z_spread)
    sc.loc[5] = sc.loc[200]; sc.vel[5] = sc.vel[200]                  # a coincident pair at rest relative to each other: NaN on both sides
    cfg = psets.config(name, use_ped_radius=rad)
    prm = O.OracleParams.from_config(cfg)
    dt = psets.step_of(name)
    geom = pc.geometry(sc)
    crossing = np.arange(n) % 9 == 0
    with np.errstate(all="ignore"):
        per, total, _ = O.tick_forces(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, crossing, geom, prm)
        v_new = O.new_velocities(sc.vel, total, sc.target_speed, dt, prm.max_speed_factor)
        cper, ctotal, cv, _, _ = c_oracle.tick(sc.loc, sc.vel, sc.waypoint, sc.target_speed, sc.radius, crossing, geom, prm, dt, nthreads=1)
    assert np.isnan(total[5]).any() and sorted(cper) == sorted(per)
    for k in per:
        _close(cper[k], per[k], f"{name}/{k}")
    _close(ctotal, total, f"{name}/total")
    _close(cv, v_new, f"{name}/new_vel")


# the scenarios of the GPU cells with N <= 1024 (tests/test_param_space_gpu.py): (n, seed, z_spread, use_ped_radius)
SMALL_CELLS = [(700, 5700, 0.0, True), (700, 5700, 1.5, True), (1000, 6000, 0.0, False), (1000, 6000, 1.5, True), (640, 6400, 0.0, True),
               (130, 7130, 0.0, True), (130, 7130, 1.5, True), (1000, 8000, 0.0, True), (1000, 8000, 1.5, True), (640, 8000, 0.0, True)]


@pytest.mark.parametrize("name", psets.NAMES)
def test_conditions_hold_on_the_oracle_alone(name):
    """Exposed rows <= 10 % and max_amp <= 1 for every set on every small cell's crowd, all five forces."""
    shares, amps = [], []
    for n, seed, z, rad in SMALL_CELLS:
        sc = pc.scene(n, seed, z)
        ref = pc.Ref(sc.loc, sc.vel, sc, pc.set_config(name, pc.ALL5, rad=rad), psets.step_of(name))
        s, a = ref.conditions(f"{name} N={n} seed {seed} z={z}")
        shares.append(s); amps.append(a)
    print(f"\n{name}: exposed share {min(shares):.1%} .. {max(shares):.1%}, max_amp {min(amps):.3g} .. {max(amps):.3g}")


@pytest.mark.parametrize("name", ["longrange", "shortrange", "epsneg"])
def test_conditions_at_the_list_cutoff_crowd(name):
    """The N = 4096 crowd of the list-cutoff cells (BASELINE config 2's generator, pedestrian + acceleration force): rows whose
    exposure exceeds ATOL <= 10 % (why not the non-zero count: _param_cells.Ref.conditions), max_amp <= 1."""
    sc, _ = scenarios.baseline_scenario("c2")
    ref = pc.Ref(sc.loc, sc.vel, sc, pc.set_config(name, pc.PED_ACC), 0.05)
    share, amp = ref.conditions(f"c2 crowd {name}", literal=False)
    print(f"\nc2 crowd {name}: rows exposed above ATOL {share:.2%}, with a non-zero exposure {ref.share:.1%}, max_amp {amp:.3g}")


def test_a_stock_reach_would_lose_terms_at_longrange():
    """Power of the list-cutoff cells.  BASELINE config 2's crowd is 128 m across; a reach from the stock gamma 0.35 / lambda 2 is
    ~65 m at |dv| = 2.8 m/s, so its list drops the tile pairs further apart -- at longrange (gamma 0.9, lambda 3) those terms are
    still ~5e-5 A each.  Per row, float64: their summed magnitude against that row's check_force allowance."""
    sc, _ = scenarios.baseline_scenario("c2")
    stock = pc.set_config("stock", pc.PED_ACC)
    powered = []
    for rows in ((0, 512), (1792, 2304), (3584, 4096)):
        power, allow = pc.stock_reach_dropped_power(sc, pc.set_config("longrange", pc.PED_ACC), stock, rows)
        powered.append(power > allow)
    share = np.concatenate(powered).mean()
    print(f"\nlongrange on the c2 crowd: a stock reach drops more than the tolerance for {share:.1%} of 1536 sampled rows")
    assert share >= 0.01


def test_a_stock_reach_loses_nothing_at_shortrange_by_construction():
    """The same sum at shortrange is zero to every digit: a stock reach is WIDER than shortrange's own (gamma 0.12 against 0.35), so a
    reach from the wrong gamma costs time there, not accuracy.  What guards shortrange is the GPU cell's count -- strictly fewer pair
    terms than the stock list on the same crowd -- and exponent underflow; this test pins the reasoning."""
    sc, _ = scenarios.baseline_scenario("c2")
    power, allow = pc.stock_reach_dropped_power(sc, pc.set_config("shortrange", pc.PED_ACC), pc.set_config("stock", pc.PED_ACC), (0, 512))
    assert (power < 1e-30).all() and (allow >= P.ATOL).all()
