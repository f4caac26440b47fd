"""SysSbaHip with the PCG solver from C++: doSBA(niter, lambda, useCSparse = 3, initTol, maxCGiters) of
include/vslam_filter_hip.hpp through examples/sba_demo.cpp --pcg."""
import os
import shutil
import subprocess

import pytest

import test_cpp_sba as base


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_sba_mirror_client_with_pcg_compiles(tmp_path):
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(base.LIBDIR, "libekfslam_hip.so")):
        g.build()
    r = base._build(str(tmp_path / "sba_demo"))
    assert r.returncode == 0, r.stderr
    src = open(base.SRC).read()
    assert "doSBA(20, 1e-4, 3, 1e-8, 100)" in src


@pytest.mark.gpu
def test_sba_mirror_client_runs_with_pcg(tmp_path):
    exe = str(tmp_path / "sba_demo")
    r = base._build(exe)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe, "--pcg"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pcg:" in run.stdout and run.stdout.strip().endswith("ok")
    bad = subprocess.run([exe, "--nope"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 64
