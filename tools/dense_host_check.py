"""Writes the case files tools/dense_host_check.cpp reads: for every exact-equality case of tests/dense_scene.py the
inputs and the outputs of tests/dense_oracle.py.  Usage: python tools/dense_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import dense_oracle as do
import dense_scene as ds

REL_TOL = 0.05


def main(out):
    os.makedirs(out, exist_ok=True)
    for (name, w, h, D, radius, trunc, src) in ds.CASES:
        views = ds.case_views(w, h)
        slots = (0,) + tuple(src)
        swept = {r: do.sweep(views[r][0], views[r][1], views[r][2], [views[s] for s in slots if s != r], ds.W_MIN, ds.W_MAX, D,
                             radius, trunc) for r in slots}
        agree = min(2, len(src))
        fd, fp = do.geometric_filter(swept[0]["depth"], swept[0]["plane"], views[0][1], views[0][2],
                                     [(swept[s]["depth"], views[s][1], views[s][2]) for s in src], REL_TOL, agree)
        with open(os.path.join(out, name + ".bin"), "wb") as fh:
            fh.write(np.array([w, h, D, radius, trunc, len(src), agree], np.int32).tobytes())
            fh.write(np.array([ds.W_MIN, ds.W_MAX, REL_TOL], np.float64).tobytes())
            for s in slots:
                fh.write(np.asarray(views[s][1], np.float64).tobytes() + np.asarray(views[s][2], np.float64).tobytes())
                fh.write(np.ascontiguousarray(views[s][0], np.uint8).tobytes())
            for s in src:
                fh.write(swept[s]["depth"].tobytes())
            for a in (swept[0]["depth"], swept[0]["plane"], swept[0]["cost"], swept[0]["views"], fd, fp,
                      do.points(swept[0]["depth"], views[0][1], views[0][2]), do.points(fd, views[0][1], views[0][2])):
                fh.write(np.ascontiguousarray(a).tobytes())
        print(name)


if __name__ == "__main__":
    main(sys.argv[1])
