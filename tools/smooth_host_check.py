"""Writes the case files tools/smooth_host_check.cpp reads: the welded meshes of tests/component_scene.py's host cases and the
two hand-made face lists of tests/smooth_oracle.py, with the oracle's adjacency and its positions and normals of four runs
(DESIGN.md §26.5).
Usage: python tools/smooth_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import component_scene as cs
import smooth_oracle as so

# (iterations, pin_boundary, normals, lam, mu)
RUNS = ((1, 0, 0, so.LAM, so.MU), (2, 1, 1, so.LAM, so.MU), (10, 0, 1, so.LAM, so.MU), (3, 0, 1, so.LAM, 0.0))


def cases():
    """name -> mesh (None: the empty one)."""
    out = {name: (None if case is None else cs.oracle_mesh(case, mc)) for name, (case, mc) in cs.host_check_cases().items()}
    out["fan40"] = so.fan_mesh()
    out["edge3"] = so.three_on_an_edge_mesh()
    return out


def names():
    return sorted(cases())


def write(path, m):
    """ints n_vert n_tri n_runs; the mesh: xyz, faces (uint32); the oracle: inc, deg (uint32), boundary (uint8); then per run:
    iterations, pin_boundary and normals (int32), lam and mu (float64), its positions and, with normals, its normals."""
    if m is None:
        m = dict(vertices=np.zeros((0, 3)), faces=np.zeros((0, 3), np.int64))
    nv, nt = len(m["vertices"]), len(m["faces"])
    adj = so.adjacency(m["faces"], nv)
    with open(path, "wb") as fh:
        fh.write(np.array([nv, nt, len(RUNS)], np.int32).tobytes())
        fh.write(np.ascontiguousarray(m["vertices"], np.float64).tobytes() + np.ascontiguousarray(m["faces"]).astype(np.uint32).tobytes())
        fh.write(adj.inc.tobytes() + adj.deg.tobytes() + adj.boundary.tobytes())
        for it, pin, nrm, lam, mu in RUNS:
            s = so.smooth(m, it, lam, mu, bool(pin), bool(nrm))
            fh.write(np.array([it, pin, nrm], np.int32).tobytes() + np.array([lam, mu], np.float64).tobytes())
            fh.write(np.ascontiguousarray(s["vertices"], np.float64).tobytes())
            if nrm:
                fh.write(np.ascontiguousarray(s["normals"], np.float32).tobytes())
    print(os.path.basename(path), nv, "vertices", nt, "triangles", int(adj.boundary.sum()), "boundary vertices")


def main(out):
    os.makedirs(out, exist_ok=True)
    for name, m in cases().items():
        write(os.path.join(out, name + ".bin"), m)


if __name__ == "__main__":
    main(sys.argv[1])
