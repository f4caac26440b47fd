"""Writes the case files tools/mesh_host_check.cpp reads: the volumes of tests/mesh_scene.py with the welded mesh of
tests/mesh_oracle.py.  Usage: python tools/mesh_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import fusion_oracle as fo
import mesh_oracle as mo
import mesh_scene as ms


def names():
    return sorted(ms.host_check_cases())


def write(path, vol, dims, origin, voxel, min_count):
    """ints nx ny nz min_count colour; doubles origin voxel; the planes sum, cnt, gsum (and csum); the oracle: n_vert and n_tri
    (uint64), xyz, key, grey (and bgr), normal (float32), faces (uint32)."""
    _, soup_key, _, _ = fo.extract(vol[:3], dims, origin, voxel, min_count)
    m = mo.weld(vol, dims, origin, voxel, soup_key, min_count, True)
    with open(path, "wb") as fh:
        fh.write(np.array(list(dims) + [min_count, int(len(vol) > 3)], np.int32).tobytes())
        fh.write(np.array(list(origin) + [voxel], np.float64).tobytes())
        for p in vol:
            fh.write(np.ascontiguousarray(p).tobytes())
        fh.write(np.array([len(m["key"]), len(m["faces"])], np.uint64).tobytes())
        fh.write(m["vertices"].tobytes() + m["key"].tobytes() + m["grey"].tobytes())
        if len(vol) > 3:
            fh.write(m["colour"].tobytes())
        fh.write(m["normals"].tobytes() + m["faces"].astype(np.uint32).tobytes())
    print(os.path.basename(path), len(m["key"]), "vertices", len(m["faces"]), "triangles")


def main(out):
    os.makedirs(out, exist_ok=True)
    for name, case in ms.host_check_cases().items():
        write(os.path.join(out, name + ".bin"), *case)


if __name__ == "__main__":
    main(sys.argv[1])
