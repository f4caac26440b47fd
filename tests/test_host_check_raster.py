"""The four kernel bodies of the rasteriser (csrc/ekf_mesh_raster.hpp: k_rast_project, k_rast_small, k_rast_large,
k_rast_resolve) run on the host under AddressSanitizer and UBSan against tests/raster_oracle.py (tools/raster_host_check.*;
DESIGN.md §30.5), built as tests/test_host_check_texture.py builds its check: a program of its own, 256 real threads a
workgroup, every buffer of exactly the size the device path gives it.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_raster_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """Depth, normal, grey, colour, triangle, barycentrics and cover equal the oracle bit for bit at small_limit 0, 64 and 65536
    on every hand-built scene (the fan also from behind, the clip scene also without its near plane), on the sphere's weld from
    pose B with both sides, at 116 x 92 from an axis, and with atlases of P = 2 with 3 channels and P = 8 with 1; the sanitizers
    report nothing: no vertex, triangle, pixel, list entry or tap out of range."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("raster_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "raster_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "raster_host_check.cpp"), "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    assert [os.path.basename(f) for f in files] == sorted(n + ".bin" for n in hc.names()) and len(files) == 15
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    print("raster: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    out = run.stdout
    # the cases are the oracle's, and both paths ran: limit 0 defers every kept triangle, 64 the large ones, 65536 none
    assert all(k in out for k in ("903 vertices, 301 triangles, 64 x 48, 3072 hit, deferred 301 1 0",
                                  "1298 vertices, 2592 triangles, 116 x 92, 4830 hit, deferred 780 32 0",
                                  "1298 vertices, 2592 triangles, 29 x 23, 270 hit, deferred 974 0 0",
                                  "9 vertices, 8 triangles, 17 x 17, 162 hit, deferred 8 0 0",
                                  "3 vertices, 1 triangles, 1 x 1, 1 hit, deferred 1 0 0"))
