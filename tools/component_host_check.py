"""Writes the case files tools/component_host_check.cpp reads: the welded meshes of tests/component_scene.py (with normals, the
wave volumes with colour) and the labels, sizes and pruned meshes of tests/component_oracle.py.
Usage: python tools/component_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import component_oracle as co
import component_scene as cs


def names():
    return sorted(cs.host_check_cases())


def _rows(fh, m, colour):
    fh.write(m["vertices"].tobytes() + m["key"].tobytes() + m["grey"].tobytes())
    if colour:
        fh.write(m["colour"].tobytes())
    fh.write(m["normals"].tobytes() + np.ascontiguousarray(m["faces"]).astype(np.uint32).tobytes())


def write(path, case, min_count):
    """ints n_vert n_tri colour n_prunes; the weld: xyz, key, grey (and bgr), normal, faces (uint32); the oracle: label, size,
    n_comp (uint64); then per prune: min_triangles and largest (uint32), n_vert, n_tri and n_kept (uint64) and its rows."""
    if case is None:
        m = dict(vertices=np.zeros((0, 3)), key=np.zeros(0, np.uint64), grey=np.zeros(0, np.uint8), colour=None,
                 normals=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int64))
    else:
        m = cs.oracle_mesh(case, min_count, True)
    colour = m["colour"] is not None
    nv, nt = len(m["key"]), len(m["faces"])
    label, size, count = co.components(m["faces"], nv)
    top = int(size.max()) if nv else 0
    prunes = [(t, False) for t in cs.THRESHOLDS + (top + 1,)] + [(1, True)]
    with open(path, "wb") as fh:
        fh.write(np.array([nv, nt, int(colour), len(prunes)], np.int32).tobytes())
        _rows(fh, m, colour)
        fh.write(label.tobytes() + size.tobytes() + np.array([count], np.uint64).tobytes())
        for min_triangles, largest in prunes:
            p = co.prune(m, min_triangles, largest)
            fh.write(np.array([min_triangles, int(largest)], np.uint32).tobytes())
            fh.write(np.array([len(p["key"]), len(p["faces"]), p["components"]], np.uint64).tobytes())
            _rows(fh, p, colour)
    print(os.path.basename(path), nv, "vertices", nt, "triangles", count, "components")


def main(out):
    os.makedirs(out, exist_ok=True)
    for name, (case, min_count) in cs.host_check_cases().items():
        write(os.path.join(out, name + ".bin"), case, min_count)


if __name__ == "__main__":
    main(sys.argv[1])
