"""Writes the case files tools/simplify_host_check.cpp reads: the welded meshes of tests/component_scene.py's host cases (with
normals, and with colour where the volume has it) and the hand-made meshes of tests/simplify_oracle.py, each with the oracle's
result at several cell sizes.
Usage: python tools/simplify_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import component_scene as cs
import simplify_oracle as so

FACTORS = (1.0, 2.0, 3.5)


def cases():
    """name -> (mesh or None: the empty one, origin, dims, voxel, cell sizes)."""
    out = {}
    for name, (case, mc) in cs.host_check_cases().items():
        _, dims, origin, voxel, _, _ = cs.cases()[case or "main"]
        out[name] = (None if case is None else cs.oracle_mesh(case, mc, True), origin, dims, voxel, tuple(f * voxel for f in FACTORS))
    hand = (so.HAND_ORIGIN, so.HAND_DIMS, so.HAND_VOXEL)
    out["opposite"] = (so.opposite_winding_mesh(),) + hand + ((1.0,),)
    out["fan40"] = (so.fan_mesh(),) + hand + ((1.0, 2.0),)
    out["outside"] = (so.outside_mesh(),) + hand + ((1.0, 1.0e9),)               # 1e9: G = (1, 1, 1)
    return out


def names():
    return sorted(cases())


def write(path, m, origin, dims, voxel, cells):
    """ints n_vert n_tri has_bgr has_normal n_runs dims[3]; float64 origin[3] voxel; the mesh: xyz, faces (uint32), grey, bgr,
    normal; then per run: float64 cell, ints n_vert_out n_tri_out n_degenerate n_duplicate G[3], and the oracle's xyz, faces
    (uint32), grey, bgr, normal, key (uint64) and map (uint32)."""
    if m is None:
        m = dict(vertices=np.zeros((0, 3)), faces=np.zeros((0, 3), np.int64), grey=np.zeros(0, np.uint8), colour=None, normals=None)
    nv, nt = len(m["vertices"]), len(m["faces"])
    bgr, nrm = m["colour"] is not None, m["normals"] is not None
    opt = lambda a, t: b"" if a is None else np.ascontiguousarray(a, t).tobytes()
    longest = 0
    with open(path, "wb") as fh:
        fh.write(np.array([nv, nt, bgr, nrm, len(cells)] + list(dims), np.int32).tobytes())
        fh.write(np.array(list(origin) + [voxel], np.float64).tobytes())
        fh.write(np.ascontiguousarray(m["vertices"], np.float64).tobytes() + np.ascontiguousarray(m["faces"]).astype(np.uint32).tobytes())
        fh.write(np.ascontiguousarray(m["grey"], np.uint8).tobytes() + opt(m["colour"], np.uint8) + opt(m["normals"], np.float32))
        for cell in cells:
            s = so.simplify(m, origin, dims, voxel, cell)
            fh.write(np.array([cell], np.float64).tobytes())
            fh.write(np.array([len(s["key"]), len(s["faces"]), s["n_degenerate"], s["n_duplicate"]] + list(s["grid"]), np.int32).tobytes())
            fh.write(s["vertices"].tobytes() + s["faces"].astype(np.uint32).tobytes() + s["grey"].tobytes() + opt(s["colour"], np.uint8))
            fh.write(opt(s["normals"], np.float32) + s["key"].tobytes() + s["map"].tobytes())
            longest = max(longest, int(np.bincount(s["cells"]).max()) if nv else 0)
    print(os.path.basename(path), nv, "vertices", nt, "triangles, longest member list", longest)


def main(out):
    os.makedirs(out, exist_ok=True)
    for name, (m, origin, dims, voxel, cells) in cases().items():
        write(os.path.join(out, name + ".bin"), m, origin, dims, voxel, cells)


if __name__ == "__main__":
    main(sys.argv[1])
