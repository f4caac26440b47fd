"""Writes the case files tools/census_host_check.cpp reads: the descriptor, sweep and semi-global cases of
tests/census_scene.py with the outputs of tests/census_oracle.py.
Usage: python tools/census_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import census_oracle as co
import census_scene as cs
import dense_scene as ds

DESCRIPTOR, SWEEP, SGM = 0, 1, 2
IDENTITY = (np.array([1.0, 1.0, 0.0, 0.0]), ds.REF)


def names():
    return (["census_" + c[0] for c in cs.DESCRIPTOR_CASES] + ["sweep_" + c[0] for c in cs.SWEEP_CASES] +
            ["sgm_" + c[0] for c in cs.SGM_CASES])


def _write(path, kind, w, h, D, radius, trunc, p1, p2, paths, views, arrays):
    with open(path, "wb") as fh:
        fh.write(np.array([kind, w, h, D, radius, trunc, len(views) - 1, p1, p2, paths], np.int32).tobytes())
        fh.write(np.array([ds.W_MIN, ds.W_MAX], np.float64).tobytes())
        for img, K, pose in views:
            fh.write(np.asarray(K, np.float64).tobytes() + np.asarray(pose, np.float64).tobytes())
            fh.write(np.ascontiguousarray(img, np.uint8).tobytes())
        for a in arrays:
            fh.write(np.ascontiguousarray(a).tobytes())


def main(out):
    os.makedirs(out, exist_ok=True)
    for case in cs.DESCRIPTOR_CASES:
        img = cs.descriptor_image(case)
        _write(os.path.join(out, "census_%s.bin" % case[0]), DESCRIPTOR, case[1], case[2], 2, 0, 1, 1, 1, 4, [(img,) + IDENTITY],
               [co.census(img)])
    for name, w, h, D, radius, trunc, src in cs.SWEEP_CASES:
        views = cs.exposed(ds.case_views(w, h))
        order = [views[s] for s in (0,) + tuple(src)]
        want = co.sweep(order[0][0], order[0][1], order[0][2], order[1:], ds.W_MIN, ds.W_MAX, D, radius, trunc)
        _write(os.path.join(out, "sweep_%s.bin" % name), SWEEP, w, h, D, radius, trunc, 1, 1, 4, order,
               [want[k] for k in ("depth", "plane", "cost", "views")])
    for case in cs.SGM_CASES:
        name, w, h, D, radius, trunc, src, p1, p2, paths, _ = case
        views = cs.exposed(cs.sgm_case_views(case))
        order = [views[s] for s in (0,) + tuple(src)]
        want = co.sweep_sgm(order[0][0], order[0][1], order[0][2], order[1:], ds.W_MIN, ds.W_MAX, D, radius, trunc, p1, p2, paths)
        _write(os.path.join(out, "sgm_%s.bin" % name), SGM, w, h, D, radius, trunc, p1, p2, paths, order,
               [want[k] for k in ("C", "S", "depth", "plane", "cost", "views")])
    for n in names():
        print(n)


if __name__ == "__main__":
    main(sys.argv[1])
