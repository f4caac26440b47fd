"""Writes the case files tools/speckle_host_check.cpp reads: the host cases of tests/speckle_scene.py with the four maps of
tests/speckle_oracle.py.
Usage: python tools/speckle_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import speckle_oracle as so
import speckle_scene as sc


def names():
    return ["speckle_" + c[0] for c in sc.HOST_CASES]


def main(out):
    os.makedirs(out, exist_ok=True)
    for case in sc.HOST_CASES:
        name, w, h, _, max_diff, min_size = case
        plane = sc.plane_map(case)
        depth = sc.depth_map(plane)
        want = so.speckle_filter(depth, plane, min_size, max_diff)
        with open(os.path.join(out, "speckle_%s.bin" % name), "wb") as fh:
            fh.write(np.array([w, h, min_size, max_diff], np.int32).tobytes())
            fh.write(np.ascontiguousarray(depth).tobytes() + np.ascontiguousarray(plane).tobytes())
            for k in ("depth", "plane", "label", "size"):
                fh.write(np.ascontiguousarray(want[k]).tobytes())
    for n in names():
        print(n)


if __name__ == "__main__":
    main(sys.argv[1])
