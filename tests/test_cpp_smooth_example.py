"""TsdfVolumeHip::smooth, smoothed, adjacency and getSmoothProfile of include/vslam_filter_hip.hpp from C++
(examples/smooth_demo.cpp): built and run the way tests/test_cpp_components_example.py builds and runs its
client."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd", "lib")
SRC = os.path.join(ROOT, "examples", "smooth_demo.cpp")


def _build(out):
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", out,
           "-L", LIBDIR, "-lekfslam_hip", "-Wl,-rpath," + LIBDIR]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_smooth_client_compiles(tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(LIBDIR, "libekfslam_hip.so")):
        g.build()
    r = _build(str(tmp_path / "smooth_demo"))
    assert r.returncode == 0, r.stderr
    text = open(SRC).read()
    assert all(name in text for name in ("smooth(", "smoothed()", "adjacency()", "getSmoothProfile", "Adjacency"))


@pytest.mark.gpu
def test_smooth_client_runs(tmp_path):
    exe = str(tmp_path / "smooth_demo")
    r = _build(exe)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok") and "1298 vertices, 2592 triangles, 0 boundary vertices" in run.stdout
