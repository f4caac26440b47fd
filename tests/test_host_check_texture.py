"""The four kernel bodies of the texture atlas (csrc/ekf_mesh_texture.hpp: k_tex_project, k_tex_select, k_tex_fill,
k_tex_fallback) run on the host under AddressSanitizer and UBSan against tests/texture_oracle.py (tools/texture_host_check.*;
DESIGN.md §29.5), built as tests/test_host_check_simplify.py builds its check: a program of its own, 256 real threads a
workgroup, every buffer of exactly the size the device path gives it.  CPU only."""
import os
import shutil
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_texture_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(tmp_path):
    """The atlas, the view and the score of every triangle, the triangles every view won, n_textured and the UVs equal the
    oracle bit for bit on the sphere (1 and 3 channels, grey and colour views, P = 2, 3 and 5), the main volume (grey views into
    3 channels, min_area2 = 0.5), a colour wave volume (the fallback blends B, G, R), the simplified sphere at P = 32 (a ragged
    last workgroup, whole block rows of padding), the two sheets with a z-buffer and then without, one triangle at P = 2 and
    a mesh without any view; the sanitizers report nothing: no vertex, triangle, texel, pixel or tap out of range."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__("texture_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / "texture_host_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread",
                                os.path.join(ROOT, "tools", "texture_host_check.cpp"), "-o", exe], capture_output=True, text=True)
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
    print("texture: %d cases in %.1f s" % (len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    out = run.stdout
    # the cases are the oracle's: the views of the sphere win 842 and 345 triangles and none, the z-buffer leaves 482 of 992
    assert all(k in out for k in ("1298 vertices, 2592 triangles, atlas 180 x 3, 3 views, 2 fills, 909 textured",
                                  "1298 vertices, 2592 triangles, atlas 144 x 1, 3 views, 2 fills, 909 textured",
                                  "1298 vertices, 2592 triangles, atlas 252 x 1, 3 views, 2 fills, 909 textured",
                                  "183 vertices, 272 triangles, atlas 120 x 3, 3 views, 3 fills, 206 textured",
                                  "913 vertices, 964 triangles, atlas 154 x 3, 3 views, 2 fills, 7 textured",
                                  "111 vertices, 218 triangles, atlas 374 x 1, 3 views, 2 fills, 88 textured",
                                  "558 vertices, 992 triangles, atlas 138 x 1, 2 views, 2 fills, 992 textured",
                                  "3 vertices, 1 triangles, atlas 4 x 3, 3 views, 2 fills, 1 textured",
                                  "9 vertices, 8 triangles, atlas 10 x 3, 0 views, 0 fills, 0 textured"))
