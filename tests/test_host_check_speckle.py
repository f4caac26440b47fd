"""The four kernel bodies of the speckle filter (csrc/ekf_dense_speckle.hpp: k_speckle_label, k_speckle_merge, k_speckle_count,
k_speckle_apply) run on the host under AddressSanitizer and UBSan against tests/speckle_oracle.py (tools/speckle_host_check.*;
DESIGN.md §23.5), built as tests/test_host_check_unique.py builds its check: a program of its own, 256 real threads a
workgroup, so the union-find of a tile and the unions across the tile borders run concurrently.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_speckle_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """Label, size, depth and plane of every host case of tests/speckle_scene.py (the five small shapes and the patterns on the
    3 x 3 grid of tiles) equal the oracle bit for bit, and the sanitizers report nothing: no neighbour index out of range, no
    plane difference that overflows."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("speckle_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "speckle_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "speckle_host_check.cpp"), "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    assert [os.path.basename(f) for f in files] == sorted(n + ".bin" for n in hc.names()) and len(files) == 32
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    print("speckle: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    kinds = run.stdout
    assert all(k in kinds for k in ("1 x 1,", "1 x 70,", "70 x 1,", "32 x 16,", "33 x 17,", "70 x 37, min_size 4, max_diff 5, 1 segments",
                                    "0 border links examined", "2590 segments"))
