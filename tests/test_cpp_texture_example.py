"""TsdfVolumeHip::textureBegin, textureAddViewHost, texture, textureFinish and getTextureProfile of include/vslam_filter_hip.hpp
from C++ (examples/texture_demo.cpp): built and run the way tests/test_cpp_simplify_example.py builds and runs
its client."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd", "lib")
SRC = os.path.join(ROOT, "examples", "texture_demo.cpp")


def _build(out):
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", out,
           "-L", LIBDIR, "-lekfslam_hip", "-Wl,-rpath," + LIBDIR]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_texture_client_compiles(tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(LIBDIR, "libekfslam_hip.so")):
        g.build()
    r = _build(str(tmp_path / "texture_demo"))
    assert r.returncode == 0, r.stderr
    text = open(SRC).read()
    assert all(name in text for name in ("textureBegin(", "textureAddViewHost(", "textureFinish()", "texture()", "getTextureProfile"))


@pytest.mark.gpu
def test_texture_client_runs(tmp_path):
    exe, ppm = str(tmp_path / "texture_demo"), str(tmp_path / "atlas.ppm")
    r = _build(exe)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe, ppm], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")
    # the oracle's figures of the same sphere (tests/test_oracle_simplify.py): 218 triangles, 11 blocks of 10 texels a side
    assert "218 triangles, atlas 110 x 110 x 3" in run.stdout
    data = open(ppm, "rb").read()
    assert data.startswith(b"P6\n110 110\n255\n") and len(data) == len(b"P6\n110 110\n255\n") + 110 * 110 * 3
