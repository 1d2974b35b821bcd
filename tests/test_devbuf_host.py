"""Host test of csrc/sfm_devbuf.h, the owning wrappers of the library's device arrays, pinned blocks, events and side stream:
tests/host/devbuf_check.cpp defines the HIP calls the header uses on top of malloc / free, counts what is alive, and walks
alloc / reserve / move / swap / a failing allocator.  Built with the host C++ compiler, no HIP runtime linked, no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "carla-social-force-model_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_devbuf_check(tmp_path):
    cxx = os.environ.get("CXX") or next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (g++, c++, clang++ or $CXX)"
    exe = str(tmp_path / "devbuf_check")
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-I{CSRC}", "-o", exe,
                            os.path.join(ROOT, "tests", "host", "devbuf_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "devbuf_check ok" in run.stdout
