"""The mirror classes of include/vslam_filter_hip.hpp from C++: DenseStereoHip (examples/dense_demo.cpp), TsdfVolumeHip
(fusion_demo.cpp), its raycast / raycastView (raycast_demo.cpp), SysSbaHip and VSlamFilterHip::keyframeProjections
(sba_demo.cpp), and SysSbaHip with the PCG solver, doSBA(niter, lambda, useCSparse = 3, initTol, maxCGiters), through
sba_demo.cpp --pcg."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd", "lib")
# example -> (source, arguments of the run, what its output has to contain, a line the source has to contain)
EXAMPLES = {
    "dense": ("dense_demo", [], None, None),
    "fusion": ("fusion_demo", [], "triangles:", None),
    "raycast": ("raycast_demo", [], "hits:", None),
    "sba": ("sba_demo", [], None, None),
    "sba_pcg": ("sba_demo", ["--pcg"], "pcg:", "doSBA(20, 1e-4, 3, 1e-8, 100)"),
}


def _src(demo):
    return os.path.join(ROOT, "examples", demo + ".cpp")


def _build(demo, out):
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), _src(demo), "-o", out,
           "-L", LIBDIR, "-lekfslam_hip", "-Wl,-rpath," + LIBDIR]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("example", sorted(EXAMPLES))
def test_mirror_client_compiles(example, tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(LIBDIR, "libekfslam_hip.so")):
        g.build()
    demo, _, _, line = EXAMPLES[example]
    r = _build(demo, str(tmp_path / demo))
    assert r.returncode == 0, r.stderr
    if line:
        assert line in open(_src(demo)).read()


@pytest.mark.gpu
@pytest.mark.parametrize("example", sorted(EXAMPLES))
def test_mirror_client_runs(example, tmp_path):
    demo, args, marker, _ = EXAMPLES[example]
    exe = str(tmp_path / demo)
    r = _build(demo, exe)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")
    if marker:
        assert marker in run.stdout
    if example == "sba_pcg":
        bad = subprocess.run([exe, "--nope"], capture_output=True, text=True, timeout=120)
        assert bad.returncode == 64
