"""The kernel bodies of the census matching cost (csrc/ekf_dense_stereo.hpp: k_census, k_plane_sweep_census;
csrc/ekf_dense_sgm.hpp: k_sweep_volume_census with the unchanged path aggregation and winner) run lane by lane on the host
under AddressSanitizer and UBSan against tests/census_oracle.py (tools/census_host_check.*), built as
tests/test_host_check_sgm.py builds its check.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_census_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """A program of its own built with AddressSanitizer and UBSan, contraction off: the descriptors, the four maps and both
    volumes of every case equal the oracle bit for bit and the sanitizers report nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("census_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "census_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "census_host_check.cpp"), "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    assert [os.path.basename(f) for f in files] == sorted(n + ".bin" for n in hc.names()) and len(files) == 9 + 7 + 4
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    print(run.stdout)
    print("census: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
