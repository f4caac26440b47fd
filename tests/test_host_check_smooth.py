"""The six kernel bodies of the mesh smoothing (csrc/ekf_mesh_smooth.hpp: k_smooth_count, k_smooth_offsets, k_smooth_fill,
k_smooth_lists, k_smooth_step, k_smooth_normals) and k_tsdf_scan between them run on the host under AddressSanitizer and UBSan
against tests/smooth_oracle.py (tools/smooth_host_check.*), built as tests/test_host_check_components.py builds
its check: a program of its own, 256 real threads a workgroup, so the corners of a workgroup of k_smooth_fill reach their
cursors in an order that varies, every buffer of exactly the size the device path gives it.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_smooth_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """inc, deg and boundary, and the positions and normals of four runs ((iterations, pin_boundary, normals) = (1, 0, 0),
    (2, 1, 1), (10, 0, 1) at the defaults and (3, 0, 1) with mu = 0) of every host case of tests/component_scene.py, of the fan of
    40 triangles and of the three triangles on one edge equal the oracle bit for bit, and the sanitizers report nothing: no
    vertex, triangle, slot or block index out of range."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("smooth_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "smooth_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "smooth_host_check.cpp"), "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    assert [os.path.basename(f) for f in files] == sorted(n + ".bin" for n in hc.names()) and len(files) == 9
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    print("smoothing: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    kinds = run.stdout
    assert all(k in kinds for k in ("183 vertices, 272 triangles, longest list 8, 4 runs", "88 vertices, 120 triangles, longest list 8, 4 runs",
                                    "913 vertices, 964 triangles, longest list 6, 4 runs", "704 vertices, 970 triangles, longest list 8, 4 runs",
                                    "1020 vertices, 1792 triangles, longest list 6, 4 runs", "1298 vertices, 2592 triangles, longest list 8, 4 runs",
                                    "0 vertices, 0 triangles, longest list 0, 4 runs", "41 vertices, 40 triangles, longest list 40, 4 runs",
                                    "5 vertices, 3 triangles, longest list 3, 4 runs"))
