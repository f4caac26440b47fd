"""The stamp rule of csrc/ekf_mesh_stamp.hpp against the bookkeeping it replaced, on the host under
AddressSanitizer and UBSan (tools/mesh_stamp_check.cpp), built as tests/test_host_check_distance.py builds its check: a program of
its own.  CPU only."""
import os
import re
import shutil
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTH = 6


def test_stamps_and_the_rules_they_replaced_agree_on_every_sequence_of_operations(tmp_path):
    """Every sequence of up to six of the 22 operations (a volume change, weld, components, prune, smooth from 0 and 1, simplify
    from 0, 1 and 2, texture begin from 0..3, and the failing variants of those that make something): after every step both rules
    agree on which of sources 0..3 resolve, on the message of each that does not, and on whether the components, the adjacency,
    the smooth result, the simplify result and the texture are current.  What follows a refused operation is not walked again: it
    is what follows the shorter sequence without it.  The walk reaches a current texture of every source, so the whole chain."""
    exe, err = str(tmp_path / "mesh_stamp_check"), ""
    for cxx in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if os.path.exists(cxx) or shutil.which(cxx):
            b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                os.path.join(ROOT, "tools", "mesh_stamp_check.cpp"), "-o", exe], capture_output=True, text=True)
            err += b.stderr
            if b.returncode == 0:
                break
    else:
        pytest.fail("no compiler built the check:\n" + err)
    t0 = time.perf_counter()
    run = subprocess.run([exe, str(LENGTH)], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    print("mesh stamps: %.1f s" % (time.perf_counter() - t0))
    assert run.returncode == 0 and run.stdout.strip().endswith("ok") and "DIFFERS" not in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    out = run.stdout
    assert "22 operations, sequences of up to %d: " % LENGTH in out
    # nothing vacuous: every source resolved, every message was given, and a texture of every source was current at some step
    for line in ("resolved", "messages", "a current texture"):
        counts = [int(c) for c in re.findall(r" (\d+)(?:,|$)", next(l for l in out.splitlines() if l.startswith(line)))]
        assert len(counts) >= 4 and all(c > 0 for c in counts), out
