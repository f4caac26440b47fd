"""The four colour kernel bodies run lane by lane on the host under AddressSanitizer and UBSan (tools/host_kernels.hpp and
tools/colour_host_check.*), as tests/test_host_checks.py runs the grey ones.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

import colour_scene as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_colour_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """tools/colour_host_check.cpp, a program of its own built with AddressSanitizer and UBSan, contraction off: every output
    of every case equals the oracle bit for bit and the sanitizers report nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import colour_host_check as hc
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "colour_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread", os.path.join(ROOT, "tools", "colour_host_check.cpp"),
                                "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    assert [os.path.basename(f) for f in files] == sorted(c + ".bin" for c in cs.HOST_CHECK_CASES)
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    print(run.stdout)
    print("colour: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    # every kernel had work: some case has triangles, some view hits, and the images of k_bgr_to_grey were all seen
    import re
    seen = [tuple(int(v) for v in m) for m in re.findall(r"(\d+) triangles \(oracle \d+\), (\d+) views with (\d+) hits, (\d+) images", run.stdout)]
    assert len(seen) == len(files) and max(s[0] for s in seen) > 0 and max(s[2] for s in seen) > 0
    assert max(s[3] for s in seen) == len(cs.GREY_SHAPES + cs.TINY_GREY_SHAPES)
