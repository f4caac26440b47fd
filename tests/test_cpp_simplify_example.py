"""TsdfVolumeHip::simplify, simplified, simplifyMap and getSimplifyProfile of include/vslam_filter_hip.hpp from C++
(examples/simplify_demo.cpp): built and run the way tests/test_cpp_smooth_example.py builds and runs its
client."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd", "lib")
SRC = os.path.join(ROOT, "examples", "simplify_demo.cpp")


def _build(out):
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", out,
           "-L", LIBDIR, "-lekfslam_hip", "-Wl,-rpath," + LIBDIR]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_simplify_client_compiles(tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(LIBDIR, "libekfslam_hip.so")):
        g.build()
    r = _build(str(tmp_path / "simplify_demo"))
    assert r.returncode == 0, r.stderr
    text = open(SRC).read()
    assert all(name in text for name in ("simplify(", "simplified()", "simplifyMap()", "getSimplifyProfile", "SimplifyStats"))


@pytest.mark.gpu
def test_simplify_client_runs(tmp_path):
    exe = str(tmp_path / "simplify_demo")
    r = _build(exe)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # the oracle's figures of the same sphere (tests/test_oracle_simplify.py)
    assert run.stdout.strip().endswith("ok")
    assert "cell 1 voxel: 2592 -> 846 triangles, 1298 -> 425 vertices, 1746 degenerate, 0 duplicate" in run.stdout
    assert "cell 2 voxels: 2592 -> 218 triangles, 1298 -> 111 vertices, 2374 degenerate, 0 duplicate" in run.stdout
