"""The eight kernel bodies of the mesh-to-mesh distance (csrc/ekf_mesh_distance.hpp) and §16's k_tsdf_scan run on the host under
AddressSanitizer and UBSan against tests/distance_oracle.py (tools/distance_host_check.*), built as
tests/test_host_check_raster.py builds its check: a program of its own, 256 real threads a workgroup, every buffer of exactly the
size the device path gives it.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_distance_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """dist, tri, closest, side and the statistics' sums, maximum and counts equal the oracle bit for bit at g = 1, 5 and automatic
    on every hand-built scene and on the sphere's weld against its 2-voxel simplification, both ways; every cursor ends at its
    cell's count and every list entry is written; the sanitizers report nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("distance_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "distance_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "distance_host_check.cpp"), "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    assert [os.path.basename(f) for f in files] == sorted(n + ".bin" for n in hc.names()) and len(files) == 10
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    print("distance: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    out = run.stdout
    # the cases are the oracle's, and the grid was in use: one cell at g = 1, the cube's 5 x 1 x 1 at 5, 35^3 for the sphere's weld
    assert all(k in out for k in ("13 triangles, 18 points, cells 1 5 3, entries 13 21 13",
                                  "2592 triangles, 111 points, cells 1 125 42875, entries 2364 3930 40914",
                                  "218 triangles, 1298 points, cells 1 125 1331",
                                  "301 triangles, 301 points, cells 1 ", "301 triangles, 1 points, cells 1 "))
