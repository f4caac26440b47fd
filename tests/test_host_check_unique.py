"""The kernel bodies of the runner-up cost and the uniqueness test (csrc/ekf_dense_stereo.hpp: the four twins of the
pixel-wise sweeps and k_depth_filter_unique; csrc/ekf_dense_sgm.hpp: k_sgm_winner_unique behind the unchanged volume and path
kernels) run lane by lane on the host under AddressSanitizer and UBSan against tests/unique_oracle.py
(tools/unique_host_check.*), built as tests/test_host_check_best.py builds its check.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unique_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """A program of its own built with AddressSanitizer and UBSan, contraction off: the five maps of every sweep case of
    tests/unique_scene.py and the filtered maps of the flat-plane scene at u = 5, 30, 100 equal the oracle bit for bit and the
    sanitizers report nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("unique_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "unique_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "unique_host_check.cpp"), "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    assert [os.path.basename(f) for f in files] == sorted(n + ".bin" for n in hc.names()) and len(files) == 23
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    print("unique: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    kinds = run.stdout
    assert all(k in kinds for k in ("census, aggregated", "absolute differences, aggregated", "best 1, absolute differences,",
                                    "best 2, census,", "best 0, census,", "best 0, absolute differences,", "uniqueness 100"))
