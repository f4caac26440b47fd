"""Writes the case files tools/sgm_host_check.cpp reads: for every exact-equality case of tests/sgm_scene.py the inputs
and the outputs of tests/sgm_oracle.py.  Usage: python tools/sgm_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import dense_scene as ds
import sgm_scene as ss


def main(out):
    os.makedirs(out, exist_ok=True)
    for case in ss.CASES + ss.MANY_PLANES_CASES:
        name, w, h, D, radius, trunc, src, p1, p2, paths, _ = case
        views = ss.case_views(case)
        want = ss.case_oracle(case)
        with open(os.path.join(out, name + ".bin"), "wb") as fh:
            fh.write(np.array([w, h, D, radius, trunc, len(src), p1, p2, paths], np.int32).tobytes())
            fh.write(np.array([ds.W_MIN, ds.W_MAX], np.float64).tobytes())
            for s in (0,) + tuple(src):
                fh.write(np.asarray(views[s][1], np.float64).tobytes() + np.asarray(views[s][2], np.float64).tobytes())
                fh.write(np.ascontiguousarray(views[s][0], np.uint8).tobytes())
            for key in ("C", "S", "depth", "plane", "cost", "views"):
                fh.write(np.ascontiguousarray(want[key]).tobytes())
        print(name)


if __name__ == "__main__":
    main(sys.argv[1])
