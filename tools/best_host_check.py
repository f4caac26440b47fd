"""Writes the case files tools/best_host_check.cpp reads: the cases of tests/best_scene.py with the outputs of
tests/best_oracle.py.
Usage: python tools/best_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import best_scene as bs
import dense_scene as ds


def names():
    return ["best_" + c[0] for c in bs.CASES]


def main(out):
    os.makedirs(out, exist_ok=True)
    for case in bs.CASES:
        name, w, h, D, radius, trunc, src, n_best, census, paths, p1, p2 = case
        views, want = bs.case_oracle(case)
        with open(os.path.join(out, "best_%s.bin" % name), "wb") as fh:
            fh.write(np.array([w, h, D, radius, trunc, len(src), n_best, census, paths, p1, p2], np.int32).tobytes())
            fh.write(np.array([ds.W_MIN, ds.W_MAX], np.float64).tobytes())
            for s in (0,) + tuple(src):
                img, K, pose = views[s]
                fh.write(np.asarray(K, np.float64).tobytes() + np.asarray(pose, np.float64).tobytes())
                fh.write(np.ascontiguousarray(img, np.uint8).tobytes())
            for k in (("C", "S") if paths else ()) + ("depth", "plane", "cost", "views"):
                fh.write(np.ascontiguousarray(want[k]).tobytes())
    for n in names():
        print(n)


if __name__ == "__main__":
    main(sys.argv[1])
