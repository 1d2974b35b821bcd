"""CPU-side checks of the drop-in boundary: libsfm_hip.so loads and exports every symbol the header
declares, and fails loudly (no CPU fallback) when no GPU is present."""
import ctypes
import os
import re

import pytest

from carla_social_force_model_amd import _lib
from carla_social_force_model_amd.config import default_sfm_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sfm_hip.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sfm_[a-z_0-9]+)\s*\(", src)))


def test_header_and_binding_agree():
    assert _declared() == sorted(_lib.SYMBOLS)


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), "libsfm_hip.so not built: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), name
    assert _lib.load().sfm_abi_version() == _lib.ABI_VERSION


def test_params_struct_layout_matches_header():
    # 4 scalars + 5 flags + 3 x 7 interaction floats + 2 border floats, all 4-byte
    assert ctypes.sizeof(_lib.SfmParamsC) == 4 * (4 + 5 + 21 + 2)
    assert ctypes.sizeof(_lib.SfmInteraction) == 28


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from carla_social_force_model_amd.engine import SfmEngine
    with pytest.raises(_lib.SfmLibraryError):
        SfmEngine(default_sfm_config(), 0.05)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "carla-social-force-model_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "sfm_oracle" not in txt, f


def test_parameters_the_formulas_cannot_honour_are_refused():
    """a decay length <= 0 of an enabled force and non-finite integration constants are refused by
    sfm_create with a message that names the parameter -- before any device is touched, so this runs without a GPU."""
    from carla_social_force_model_amd.engine import params_from_config
    lib = _lib.load()
    for mutate, word in ((lambda p: setattr(p.pedestrian, "gamma", -0.35), "pedestrian_force.gamma"),
                         (lambda p: setattr(p.pedestrian, "gamma", 0.0), "pedestrian_force.gamma"),
                         (lambda p: setattr(p, "border_b", -0.3), "border_force.b"),
                         (lambda p: setattr(p.static_obstacle, "gamma", -0.4), "static_obstacle_force.gamma"),
                         (lambda p: setattr(p.dynamic_obstacle, "gamma", float("nan")), "dynamic_obstacle_force.gamma"),
                         (lambda p: setattr(p, "tau", float("inf")), "tau"),
                         (lambda p: setattr(p, "tau", 0.0), "tau"),
                         (lambda p: setattr(p, "max_speed_factor", float("nan")), "max_speed_factor"),
                         (lambda p: setattr(p, "step_length", float("inf")), "step_length")):
        p = params_from_config(default_sfm_config(), 0.05)
        mutate(p)
        h = ctypes.c_void_p()
        assert lib.sfm_create(ctypes.byref(p), 0, ctypes.byref(h)) == -1 and not h.value, word
        assert word in lib.sfm_last_error(None).decode(), (word, lib.sfm_last_error(None))
    # ... and a force that is switched off is not looked at: the refusal then comes from the missing device, not the parameter
    p = params_from_config(default_sfm_config(("acceleration_force", "pedestrian_force")), 0.05)
    p.border_b = -1.0
    h = ctypes.c_void_p()
    rc = lib.sfm_create(ctypes.byref(p), 0, ctypes.byref(h))
    assert rc == 0 or "border_force" not in lib.sfm_last_error(None).decode()
    if rc == 0:
        lib.sfm_destroy(h)
