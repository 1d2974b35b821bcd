"""Named parameter sets away from the stock sfm_config.toml, shared by tests/golden/make_golden.py (reference fixtures
``ps_*.npz``), the host tests and tests/test_param_space_gpu.py.  Data only.

The kernels do not evaluate the formulas with the parameters as given: the host folds them into derived constants (eps gamma,
-log2e / gamma, (n gamma)^2 log2e, ...) and into reach bounds that decide which work is skipped (cut_scale from the pedestrian
gamma, border_skip from border b).  At the stock values the skipped terms are exactly negligible; each set below moves the
parameters so that a constant or a bound derived from the wrong value shows:

  longrange   reach and skip distances that must GROW with gamma, lambda, b
  shortrange  exponent underflow, ex2 of very negative arguments, large A / a, use_ped_radius making d - r negative
  eps0        theta no longer biased off 0: the sign(theta) / copysign paths
  epsneg      sign assumptions on the bias, n > n' (k1 / k2 swapped)
  lam0        D = e exactly; the three interactions' constants told apart (thresholds, gamma, n all differ)
  integrate   tau, max_speed_factor and the step length, which no other fixture moves

``STEP[name]`` is the set's step length (the generator's 0.05 unless the set moves it)."""
import copy

from carla_social_force_model_amd.config import default_sfm_config

SETS = {
    "longrange": {"pedestrian_force": {"gamma": 0.9, "lambda": 3.0, "A": 2.0}, "border_force": {"b": 1.5, "a": 2.0}},
    "shortrange": {"pedestrian_force": {"gamma": 0.12, "lambda": 0.5, "A": 20.0, "n": 1.0, "n_prime": 1.5},
                   "border_force": {"b": 0.05, "a": 12.0}},
    "eps0": {"pedestrian_force": {"epsilon": 0.0}, "static_obstacle_force": {"epsilon": 0.0},
             "dynamic_obstacle_force": {"epsilon": 0.0}},
    "epsneg": {"pedestrian_force": {"epsilon": -0.05, "n": 3.5, "n_prime": 0.5}},
    "lam0": {"pedestrian_force": {"lambda": 0.0},
             "static_obstacle_force": {"lambda": 0.0, "perception_threshold": 7},
             "dynamic_obstacle_force": {"perception_threshold": 11, "gamma": 0.8, "n": 2.5}},
    "integrate": {"goal_force": {"tau": 0.25}, "max_speed_factor": 2.0},
    # the same tables, at the finer of the two step lengths
    "integrate_fine": {"goal_force": {"tau": 0.25}, "max_speed_factor": 2.0},
}
STEP = {"integrate": 0.1, "integrate_fine": 0.0125}
DEFAULT_STEP = 0.05
NAMES = ("longrange", "shortrange", "eps0", "epsneg", "lam0", "integrate")      # the six sets of the table
FORCE_SETS = ("longrange", "shortrange", "eps0", "epsneg", "lam0")             # ... those that move a force


def step_of(name):
    return STEP.get(name, DEFAULT_STEP)


def config(name, forces=None, use_ped_radius=False):
    """The stock config with set ``name`` laid over it (``name`` None or 'stock': the stock config itself)."""
    cfg = default_sfm_config(forces)
    for key, val in ({} if name in (None, "stock") else SETS[name]).items():
        if isinstance(val, dict):
            cfg.setdefault(key, {}).update(copy.deepcopy(val))
        else:
            cfg[key] = val
    cfg["use_ped_radius"] = bool(use_ped_radius)
    return cfg
