"""The four kernel bodies of the device weld (csrc/ekf_mesh.hpp: k_mesh_cells, k_mesh_edges, k_mesh_vertices with and without
normals, k_mesh_faces) and k_tsdf_scan between them run on the host under AddressSanitizer and UBSan against
tests/mesh_oracle.py (tools/mesh_host_check.*), built as tests/test_host_check_speckle.py builds its check: a
program of its own, 256 real threads a workgroup, every buffer of exactly the size the device path gives it.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mesh_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """Vertices, keys, grey, colour, normals and faces of every host case of tests/mesh_scene.py equal the oracle bit for bit, and
    the sanitizers report nothing: no cell, neighbour or vertex index out of range."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("mesh_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "mesh_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "mesh_host_check.cpp"), "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    assert [os.path.basename(f) for f in files] == sorted(n + ".bin" for n in hc.names()) and len(files) == 13
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    print("mesh: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    kinds = run.stdout
    assert all(k in kinds for k in ("2 x 2 x 2,", "3 x 2 x 2,", "257 x 2 x 2,", "16 x 16 x 3,", "19 x 13 x 11, min_count 1, grey, 183 vertices",
                                    "17 x 15 x 13, min_count 1, grey, 1298 vertices", " 0 vertices, 0 triangles", "colour"))
