"""Host test of csrc/sfm_metres.h, the one check of a per-scene length in metres behind sfm_batch_set_observation, _set_episodes
and _set_scan: tests/host/metres_check.cpp walks 0, -0, the smallest denormal, 1, 1e6, the float above 1e6, +-inf, -1 and NaN in both
strictness modes -- accepted or refused, the exact message, the square formed in double and rounded once -- and a few hundred
thousand lengths in between.  Built with the host C++ compiler, no HIP runtime linked, no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "carla-social-force-model_amd", "csrc")


def test_metres_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (g++, c++, clang++ or $CXX)"
    exe = str(tmp_path / "metres_check")
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-O1", f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", "-o", exe,
                            os.path.join(ROOT, "tests", "host", "metres_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "metres_check ok" in run.stdout
