"""The seven kernel bodies of the mesh components (csrc/ekf_mesh_components.hpp: k_comp_init, k_comp_union, k_comp_count,
k_comp_largest, k_comp_flags, k_comp_vertices, k_comp_faces) and k_tsdf_scan between them run on the host under
AddressSanitizer and UBSan against tests/component_oracle.py (tools/component_host_check.*), built as
tests/test_host_check_speckle.py builds its check: a program of its own, 256 real threads a workgroup, so the unions of a
workgroup run concurrently, every buffer of exactly the size the device path gives it.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_component_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """Labels, sizes, the number of components and six pruned meshes (min_triangles 1, 3, 9, 41, one above the largest size, and
    the largest component) of every host case of tests/component_scene.py equal the oracle bit for bit, and the sanitizers
    report nothing: no vertex, triangle or block index out of range."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("component_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "component_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "component_host_check.cpp"), "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    assert [os.path.basename(f) for f in files] == sorted(n + ".bin" for n in hc.names()) and len(files) == 7
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    print("components: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    kinds = run.stdout
    assert all(k in kinds for k in ("183 vertices, 272 triangles, grey, 3 components", "88 vertices, 120 triangles, grey, 2 components",
                                    "913 vertices, 964 triangles, colour, 58 components", "704 vertices, 970 triangles, colour, 11 components",
                                    "1020 vertices, 1792 triangles, grey, 4 components", "1298 vertices, 2592 triangles, grey, 1 components",
                                    "0 vertices, 0 triangles, grey, 0 components"))
