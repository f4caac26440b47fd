"""The kernel bodies of the semi-global sweep (csrc/ekf_dense_sgm.hpp: the volume sweep, the path aggregation with its
cross-lane reads emulated by tools/host_kernels.hpp, the winner) run lane by lane on the host under AddressSanitizer and
UBSan against tests/sgm_oracle.py (tools/sgm_host_check.*), built as tests/test_host_checks.py builds the
other checks.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

import sgm_scene as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sgm_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """A program of its own built with AddressSanitizer and UBSan, contraction off: both volumes and the four maps of
    every case equal the oracle bit for bit and the sanitizers report nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("sgm_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "sgm_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "sgm_host_check.cpp"), "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    assert [os.path.basename(f) for f in files] == sorted(c[0] + ".bin" for c in ss.CASES + ss.MANY_PLANES_CASES)
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    print(run.stdout)
    print("sgm: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
