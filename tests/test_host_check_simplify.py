"""The nine kernel bodies of the mesh simplification (csrc/ekf_mesh_simplify.hpp: k_simp_cells, k_simp_count, k_simp_offsets,
k_simp_fill, k_simp_lists, k_simp_flags, k_simp_map, k_simp_vertices, k_simp_faces) and k_tsdf_scan between them run on the host
under AddressSanitizer and UBSan against tests/simplify_oracle.py (tools/simplify_host_check.*), built as
tests/test_host_check_smooth.py builds its check: a program of its own, 256 real threads a workgroup, so the vertices and
triangles of a workgroup of k_simp_fill reach their cursors in an order that varies, every buffer of exactly the size the device
path gives it.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_simplify_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """The grid, the four counts, every row of the result and the vertex map of every host case of tests/component_scene.py
    (with normals, the wave volumes with colour) at cell = 1, 2 and 3.5 voxels, of the two triangles of opposite winding and of
    the vertices outside the box (at 1 voxel and at a cell so large that G = (1, 1, 1)) and of the fan of 54 triangles under one least cell equal the oracle bit for bit, and the
    sanitizers report nothing: no vertex, triangle, cell, slot or block index out of range."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("simplify_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "simplify_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "simplify_host_check.cpp"), "-o", exe], capture_output=True, text=True)
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
    print("simplification: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    kinds = run.stdout
    # the longest member lists are the oracle's: 27 of the main volume, 93 of the sphere and 98 of the four sheets at 3.5 voxels,
    # beyond the insertion sort's 16, so the heap sort runs; every vertex of `outside` in one cell at G = (1, 1, 1)
    assert all(k in kinds for k in ("183 vertices, 272 triangles, longest member list 27, 3 runs", "88 vertices, 120 triangles, longest member list 25, 3 runs",
                                    "913 vertices, 964 triangles, longest member list 27, 3 runs", "704 vertices, 970 triangles, longest member list 65, 3 runs",
                                    "1020 vertices, 1792 triangles, longest member list 98, 3 runs", "1298 vertices, 2592 triangles, longest member list 93, 3 runs",
                                    "0 vertices, 0 triangles, longest member list 0, 3 runs", "6 vertices, 2 triangles, longest member list 2, 1 runs",
                                    "6 vertices, 2 triangles, longest member list 6, 2 runs", "41 vertices, 54 triangles, longest member list 8, 2 runs"))
