"""Writes the case files tools/distance_host_check.cpp reads: the hand-built targets and points of tests/distance_scene.py and the
sphere's weld against its 2-voxel simplification, both ways, with the oracle's result and statistics.
Usage: python tools/distance_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import distance_oracle as do
import distance_scene as ds

THR = 0.0625


def cases():
    """name -> (mesh, points)."""
    out = dict(ds.scenes())
    weld, simp = ds.sphere_weld(), ds.sphere_simplified(2.0)
    out["sphere_simplified_to_weld"] = (weld, simp["vertices"])
    out["sphere_weld_to_simplified"] = (simp, weld["vertices"])
    return out


def names():
    return sorted(cases())


def write(path, mesh, points):
    """uint32 n_vert n_tri n_pts; the mesh: xyz, faces (uint32); the points; then the oracle's dist, tri, closest, side; float64
    thr, sum, sum2, max (-1 without a finite point); uint32 argmax, within, bad."""
    r = do.distance(mesh, points)
    s = do.stats(r["dist"], THR)
    X, F = np.ascontiguousarray(mesh["vertices"], np.float64), np.ascontiguousarray(mesh["faces"]).astype(np.uint32)
    P = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    with open(path, "wb") as fh:
        fh.write(np.array([len(X), len(F), len(P)], np.uint32).tobytes())
        fh.write(X.tobytes() + F.tobytes() + P.tobytes())
        fh.write(r["dist"].tobytes() + r["tri"].tobytes() + r["closest"].tobytes() + r["side"].tobytes())
        fh.write(np.array([THR, s["sum"], s["sum2"], s["max"] if s["n"] else -1.0], np.float64).tobytes())
        fh.write(np.array([s["argmax"], s["within"], s["n_bad"]], np.uint32).tobytes())
    print(os.path.basename(path), len(F), "triangles", len(P), "points, max", s["max"], "mean", s["mean"])


def main(out):
    os.makedirs(out, exist_ok=True)
    for name, case in cases().items():
        write(os.path.join(out, name + ".bin"), *case)


if __name__ == "__main__":
    main(sys.argv[1])
