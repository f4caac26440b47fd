"""The kernel bodies of the dense, fusion and ray-casting headers, the colour kernels among them, and the patch matcher and
template blur of the image header run lane by lane on the host under AddressSanitizer and UBSan (tools/host_kernels.hpp and
tools/*_host_check.*), and
so does the filter's host bookkeeping (tools/filter_host_check.*, DESIGN.md §2: the feature table against its Python model;
read-back queue, input ring and launch profiler against stand-in HIP calls, with the runtime's API header for the types
only and no HIP library).  CPU only."""
import os
import re
import shutil
import subprocess
import sys
import time

import pytest

import colour_scene as cs
import dense_scene as ds
import fusion_scene as fs
import image_scene as isc
import raycast_scene as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cases the writer of each check is to produce, as its scene module names them
CASES = {"colour": lambda: list(cs.HOST_CHECK_CASES), "dense": lambda: [c[0] for c in ds.CASES],
         "fusion": lambda: list(fs.HOST_CHECK_CASES), "image": lambda: list(isc.HOST_CHECK_CASES), "raycast": lambda: list(rs.cases()),
         "filter": lambda: list(__import__("filter_host_check").SEQUENCES)}
# (the filter check reads the runtime's API header for its types; the others include no HIP header and build as they did)
HIP_TYPES = {"filter": ["-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_bodies_on_the_host_equal_the_oracle_under_sanitizers(name, tmp_path):
    """tools/<name>_host_check.cpp, a program of its own built with AddressSanitizer and UBSan, contraction off: every output
    of every case equals the oracle bit for bit and the sanitizers report nothing."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    hc = __import__(name + "_host_check")
    hc.main(str(tmp_path / "cases"))
    exe, err = str(tmp_path / (name + "_host_check")), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=undefined", "-pthread"] + HIP_TYPES.get(name, []) +
                               [os.path.join(ROOT, "tools", name + "_host_check.cpp"),
                                "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the host check:\n" + err)
    files = sorted(str(p) for p in (tmp_path / "cases").iterdir())
    want = CASES[name]()
    assert len(files) == len(want) and [os.path.basename(f) for f in files] == sorted(c + ".bin" for c in want)
    t0 = time.perf_counter()
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    print(run.stdout)
    print("%s: %d cases in %.1f s" % (name, len(files), time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    if name == "colour":
        # every kernel had work: some case has triangles, some view hits, and the images of k_bgr_to_grey were all seen
        seen = [tuple(int(v) for v in m) for m in re.findall(r"(\d+) triangles \(oracle \d+\), (\d+) views with (\d+) hits, (\d+) images", run.stdout)]
        assert len(seen) == len(files) and max(s[0] for s in seen) > 0 and max(s[2] for s in seen) > 0
        assert max(s[3] for s in seen) == len(cs.GREY_SHAPES + cs.TINY_GREY_SHAPES)
