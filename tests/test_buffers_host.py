"""csrc/ekf_buffers.hpp on the CPU: tests/buffers_host.cpp instantiates Buf, and IndexedMeshBufs with its all-or-nothing grow,
with a counting malloc / free allocator and is built with the host compiler under AddressSanitizer and UBSan (a stand-alone program: nothing is loaded into Python).
The header includes the HIP runtime's API header for hipError_t, so the build needs ROCm's include path, not its library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "buffers_host.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _compiler():
    """g++, else ROCm's clang++: both link and run the two sanitizers."""
    for cxx in ("g++", os.path.join(ROCM, "llvm", "bin", "clang++"), "clang++"):
        path = shutil.which(cxx)
        if path:
            # (the runtimes inside the program: it runs whatever else the loader brings; clang links them statically anyway)
            return [path] + (["-static-libasan", "-static-libubsan"] if cxx == "g++" else [])
    return None


def test_buf_ownership_under_sanitizers(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler (g++ or ROCm's clang++)"
    exe = str(tmp_path / "buffers_host")
    cmd = cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                 "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)     # (LeakSanitizer on, as by default)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "allocs=48 frees=48 ok"
