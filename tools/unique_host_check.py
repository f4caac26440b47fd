"""Writes the case files tools/unique_host_check.cpp reads: the sweep cases of tests/unique_scene.py with the five maps of
tests/unique_oracle.py, and the filter of the flat-plane scene at three values of the uniqueness.
Usage: python tools/unique_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import dense_scene as ds
import unique_scene as us

FILTER_U = (5, 30, 100)


def names():
    return ["unique_" + c[0] for c in us.CASES] + ["unique_filter_u%d" % u for u in FILTER_U]


def main(out):
    os.makedirs(out, exist_ok=True)
    for case in us.CASES:
        name, w, h, D, radius, trunc, src, census, n_best, paths, p1, p2, _ = case
        views, want = us.case_oracle(case)
        with open(os.path.join(out, "unique_%s.bin" % name), "wb") as fh:
            fh.write(np.array([0, w, h, D, radius, trunc, len(src), n_best, census, paths, p1, p2], np.int32).tobytes())
            fh.write(np.array([ds.W_MIN, ds.W_MAX], np.float64).tobytes())
            for s in (0,) + tuple(src):
                img, K, pose = views[s]
                fh.write(np.asarray(K, np.float64).tobytes() + np.asarray(pose, np.float64).tobytes())
                fh.write(np.ascontiguousarray(img, np.uint8).tobytes())
            for k in ("depth", "plane", "cost", "views", "runner"):
                fh.write(np.ascontiguousarray(want[k]).tobytes())
    scene, swept, _ = us.flat_row(us.FLAT_ROWS[0])
    for u in FILTER_U:
        fd, fp = us.flat_filter(scene, swept, u)
        with open(os.path.join(out, "unique_filter_u%d.bin" % u), "wb") as fh:
            fh.write(np.array([1, ds.W, ds.H, 2, us.FLAT_MIN_AGREE, u], np.int32).tobytes())
            fh.write(np.array([us.FLAT_REL_TOL], np.float64).tobytes())
            for s in (0, 1, 2):
                fh.write(np.asarray(scene[s][1], np.float64).tobytes() + np.asarray(scene[s][2], np.float64).tobytes())
            for k in ("depth", "plane", "cost", "runner"):
                fh.write(np.ascontiguousarray(swept[0][k]).tobytes())
            for s in (1, 2):
                fh.write(np.ascontiguousarray(swept[s]["depth"]).tobytes())
            fh.write(np.ascontiguousarray(fd).tobytes() + np.ascontiguousarray(fp).tobytes())
    for n in names():
        print(n)


if __name__ == "__main__":
    main(sys.argv[1])
