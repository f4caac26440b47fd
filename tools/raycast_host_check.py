"""Writes the case files tools/raycast_host_check.cpp reads: the GPU test shapes of tests/raycast_scene.py with the inputs and
the outputs of tests/raycast_oracle.py.  Usage: python tools/raycast_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import fusion_oracle as fo
import raycast_oracle as ro
import raycast_scene as rs


def write(path, vol, dims, origin, voxel, shape, K, pose, z_near, z_far, step, min_count):
    """ints nx ny nz W H N min_count; doubles origin voxel K pose z_near step; the three planes; the oracle: the mean plane,
    depth, normal, grey."""
    r = ro.raycast(vol, dims, origin, voxel, shape, K, pose, z_near, z_far, step, min_count)
    with open(path, "wb") as fh:
        fh.write(np.array(list(dims) + list(shape) + [r["stats"]["samples"], min_count], np.int32).tobytes())
        fh.write(np.array(list(origin) + [voxel] + list(K) + list(pose) + [z_near, step], np.float64).tobytes())
        for p in vol:
            fh.write(np.ascontiguousarray(p).tobytes())
        fh.write(ro.mean_plane(vol, min_count).tobytes() + r["depth"].tobytes() + r["normal"].tobytes() + r["grey"].tobytes())
    print(os.path.basename(path), r["stats"])


def main(out):
    os.makedirs(out, exist_ok=True)
    for name, c in rs.cases().items():
        write(os.path.join(out, name + ".bin"), **c)


if __name__ == "__main__":
    main(sys.argv[1])
